/*
 * lenv_oracle.c -- CPU ORACLE (test infrastructure; see lenv_oracle.h header comment).
 *
 * Every function cites the reference file:line (relative to /root/reference) it restates.
 * Build: gcc -O2 -ffp-contract=off -mfma -fPIC -shared -pthread (oracle/Makefile).
 * -ffp-contract=off is REQUIRED: fused multiply-adds appear only where fmaf() is written.
 */
#include "lenv_oracle.h"

#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------
 * deterministic math (no libm transcendental calls: the HIP kernels implement the same
 * polynomial sequences, so results agree bitwise between gcc/x86 and hipcc/gfx950)
 * ---------------------------------------------------------------------------------------- */

static inline float bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* Canonical tanh (v4): t = min(|x|, TMAX), u = t + 2^19 (one float addition: the ulp of 2^19 is 1/16, so the addition rounds
 * t to the nearest grid point i/16 and the low mantissa bits of u are i), i = bits(u) - bits(2^19), d = t - (u - 2^19)
 * (both differences exact, |d| <= 1/32), tanh(x) = copysign(((c3 d + c2) d + c1) d + c0, x) with (c0..c3)_i of
 * lenv_tanh_table.h = cubic fit of tanh(i/16 + d) (tools/gen_tanh_table.py; entry 0 pins c0 = 0, c1 = 1, c2 = 0).  147 entries.
 * No exp, no division, no final clamp.  On the GPU a pair of hidden units costs 15 VALU instructions + two 16-byte gathers
 * (the steps to u, u - 2^19 and d are packed adds, the LDS address is one shift-add of bits(u)); the table is small enough
 * for 16 bank-private LDS copies (conflict-free gathers).  Replaces torch.tanh (activation_fn 'tanh',
 * models/model_utils.py:15-16); max deviation from the exact tanh is 6.5e-8 absolute; every result lies in [0,1]
 * (tests/test_oracle_golden.py checks all 1.1e9 floats in [0, 16]).
 * (v3, rounds 1-2, indexed a log-spaced table by the exponent / mantissa bits of |x| + 1: 18 instructions per pair.) */
#include "lenv_tanh_table.h"
static const float orc_tanh_table[LENV_TANH_N * 4] = LENV_TANH_TABLE_INIT;

float orc_tanhf(float x)
{
    float ax = fabsf(x);
    float t = ax < LENV_TANH_TMAX ? ax : LENV_TANH_TMAX;
    float u = t + LENV_TANH_MAGIC;                      /* rounds t to the 1/16 grid (ulp of 2^19): IEEE semantics required --  */
    float r = u - LENV_TANH_MAGIC;                      /* no -ffast-math / -fassociative-math (oracle/Makefile has neither)  */
    float d = t - r;                                    /* exact, |d| <= 1/32                                                  */
    uint32_t b;
    memcpy(&b, &u, 4);
    const float *k = orc_tanh_table + 4 * (int)(b - LENV_TANH_MAGIC_BITS);
    float p = fmaf(k[3], d, k[2]);
    p = fmaf(p, d, k[1]);
    p = fmaf(p, d, k[0]);
    return copysignf(p, x);
}

/* Exhaustive range check used by the test-suite: evaluates orc_tanhf on every float whose bit pattern lies in
 * [lo_bits, hi_bits]; returns the number of results outside [0,1] or breaking monotonicity by more than `slack`. */
int64_t orc_tanhf_scan(uint32_t lo_bits, uint32_t hi_bits, float slack, float *max_out)
{
    int64_t bad = 0;
    float prev = 0.0f, mx = 0.0f;
    for (uint64_t b = lo_bits; b <= hi_bits; ++b) {
        uint32_t bb = (uint32_t)b;
        float x, y;
        memcpy(&x, &bb, 4);
        y = orc_tanhf(x);
        if (!(y >= 0.0f && y <= 1.0f)) ++bad;
        if (y < prev - slack) ++bad;
        if (y > prev) prev = y;
        if (y > mx) mx = y;
    }
    if (max_out) *max_out = mx;
    return bad;
}

/* sin/cos in double: Cody-Waite reduction by pi/2 (3 constants) + fdlibm kernel polynomials.
 * Replaces math.sin/math.cos / numpy sin/cos inside gym's CartPole/Acrobot (third party). */
static const double PIO2_1 = 1.57079632673412561417e+00;  /* first 33 bits of pi/2 */
static const double PIO2_2 = 6.07710050630396597660e-11;  /* second 33 bits */
static const double PIO2_3 = 2.02226624871116645580e-21;  /* third 33 bits */

static inline double ksin(double x)
{
    double z = x * x;
    double p = 1.58969099521155010221e-10;
    p = fma(p, z, -2.50507602534068634195e-08);
    p = fma(p, z, 2.75573137070700676789e-06);
    p = fma(p, z, -1.98412698298579493134e-04);
    p = fma(p, z, 8.33333333332248946124e-03);
    p = fma(p, z, -1.66666666666666324348e-01);
    return fma(x * z, p, x);
}

static inline double kcos(double x)
{
    double z = x * x;
    double p = -1.13596475577881948265e-11;
    p = fma(p, z, 2.08757232129817482790e-09);
    p = fma(p, z, -2.75573143513906633035e-07);
    p = fma(p, z, 2.48015872894767294178e-05);
    p = fma(p, z, -1.38888888888741095749e-03);
    p = fma(p, z, 4.16666666666666019037e-02);
    /* 1 - (z/2 - z*z*p) */
    return 1.0 - fma(-z * z, p, 0.5 * z);
}

static inline void sincos_reduce(double x, double *r, int *quadrant)
{
    double kf = rint(x * 6.36619772367581382433e-01); /* 2/pi */
    double t = fma(-kf, PIO2_1, x);
    t = fma(-kf, PIO2_2, t);
    t = fma(-kf, PIO2_3, t);
    *r = t;
    *quadrant = (int)((long long)kf & 3);
}

double orc_sin(double x)
{
    double r; int q;
    sincos_reduce(x, &r, &q);
    switch (q) {
    case 0: return ksin(r);
    case 1: return kcos(r);
    case 2: return -ksin(r);
    default: return -kcos(r);
    }
}

double orc_cos(double x)
{
    double r; int q;
    sincos_reduce(x, &r, &q);
    switch (q) {
    case 0: return kcos(r);
    case 1: return -ksin(r);
    case 2: return -kcos(r);
    default: return ksin(r);
    }
}

/* ------------------------------------------------------------------------------------------
 * counter-based RNG (production mode).  The reference draws from torch / numpy / python
 * `random` / gym np_random global streams; those cannot be
 * reproduced on a GPU, so every stochastic input is either an explicit tape (parity mode)
 * or value = hash(key, stream, n) with this 64-bit mixer (two rounds of the splitmix64 finaliser).
 * ---------------------------------------------------------------------------------------- */
uint64_t orc_mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

uint64_t orc_chain_key(uint64_t seed, uint64_t generation, uint64_t worker, uint64_t kind)
{
    uint64_t k = orc_mix64(seed + 0x9e3779b97f4a7c15ULL);
    k = orc_mix64(k ^ (generation + 0x9e3779b97f4a7c15ULL * 2));
    k = orc_mix64(k ^ (worker + 0x9e3779b97f4a7c15ULL * 3));
    k = orc_mix64(k ^ (kind + 0x9e3779b97f4a7c15ULL * 4));     /* own round: distinct for every (worker, kind) */
    return k;
}

uint64_t orc_rng_u64(uint64_t key, uint32_t stream, uint64_t n)
{
    uint64_t x = key + 0x9e3779b97f4a7c15ULL * (((uint64_t)stream << 56) ^ n);
    return orc_mix64(orc_mix64(x) ^ key);
}

enum { STREAM_EPS = 0, STREAM_ACTION = 1, STREAM_REPLAY = 2, STREAM_TRAIN_RESET = 3, STREAM_TEST_RESET = 4 };

/* ReplayBuffer.sample index draw n (utils.py:35 np.random.randint(0, size)) in counter mode: one 32-bit murmur3 finaliser
 * over (n, key), mapped to [0, size) by a multiply-high (same function in csrc/lenv_device.cuh rng_replay_below). */
uint32_t orc_rng_replay_below(uint64_t key, uint64_t n, uint32_t size)
{
    uint32_t h = (uint32_t)n * 0x9e3779b1u + (uint32_t)key;
    h ^= (uint32_t)(key >> 32);
    h ^= h >> 16; h *= 0x85ebca6bu;
    h ^= h >> 13; h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return (uint32_t)(((uint64_t)h * (uint64_t)size) >> 32);
}

static inline double u64_to_unit(uint64_t u) { return (double)(u >> 11) * (1.0 / 9007199254740992.0); }
static inline uint32_t u64_to_below(uint64_t u, uint32_t n) { return (uint32_t)(((u >> 32) * (uint64_t)n) >> 32); }

/* ------------------------------------------------------------------------------------------
 * MLP (models/model_utils.py:4-39)
 * ---------------------------------------------------------------------------------------- */
int64_t orc_mlp_num_params(const orc_mlp_desc *d)
{
    int64_t H = d->hidden;
    return (int64_t)d->in_dim * H + H + (int64_t)(d->layers - 1) * (H * H + H) + H * d->out_dim + d->out_dim
           + ((d->use_layer_norm && d->layers >= 2) ? 2 * H : 0);
}

static inline float act_fwd(int act, float prelu, float z)
{
    switch (act) {
    case ORC_ACT_RELU: return z > 0.0f ? z : 0.0f;
    case ORC_ACT_LEAKYRELU: return z > 0.0f ? z : z * 0.01f;      /* nn.LeakyReLU() default slope */
    case ORC_ACT_TANH: return orc_tanhf(z);
    case ORC_ACT_PRELU: return z > 0.0f ? z : prelu * z;
    default: return z;
    }
}

/* derivative factor applied to the upstream gradient; z = pre-activation, a = activation */
static inline float act_bwd(int act, float prelu, float z, float a, float g)
{
    switch (act) {
    case ORC_ACT_RELU: return a > 0.0f ? g : 0.0f;                /* threshold_backward */
    case ORC_ACT_LEAKYRELU: return z > 0.0f ? g : g * 0.01f;
    case ORC_ACT_TANH: return g * fmaf(-a, a, 1.0f);              /* torch CPU tanh_backward (verified bitwise) */
    case ORC_ACT_PRELU: return z > 0.0f ? g : prelu * g;
    default: return g;
    }
}

/* y[o] = (sum_k fmaf chain from 0) + b[o]  -- torch-CPU batched linear order */
static inline void linear_fwd(const float *W, const float *b, int n_out, int n_in, const float *x, float *y)
{
    for (int o = 0; o < n_out; ++o) {
        float acc = 0.0f;
        const float *w = W + (int64_t)o * n_in;
        for (int k = 0; k < n_in; ++k) acc = fmaf(x[k], w[k], acc);
        y[o] = acc + b[o];
    }
}

#define ORC_MAX_WIDTH 1024
#define ORC_MAX_LAYERS 4

/* single-sample forward keeping pre-activations z[l] (after the LayerNorm where there is one) and activations a[l]
 * (l = 0..L-1); xh / rstd (optional): the normalised rows and 1/sqrt(var + eps) of the LayerNorm positions, for the backward */
static void mlp_forward_one_ex(const orc_mlp_desc *d, const float *p, const float *x, float *y,
                               float z[][ORC_MAX_WIDTH], float a[][ORC_MAX_WIDTH], float xh[][ORC_MAX_WIDTH], float *rstd_out)
{
    const int H = d->hidden, L = d->layers;
    const float *in = x;
    int n_in = d->in_dim;
    const float *ln_w = NULL, *ln_b = NULL;
    for (int l = 0; l < L; ++l) {
        const float *W = p; p += (int64_t)H * n_in;
        const float *b = p; p += H;
        linear_fwd(W, b, H, n_in, in, z[l]);
        if (d->use_layer_norm && l >= 1) {
            /* nn.LayerNorm(hidden), eps 1e-5, biased variance: sequential sums, y = fma((z - mean) * rstd, w, b) */
            if (l == 1) { ln_w = p; ln_b = p + H; p += 2 * H; }
            float sm = 0.0f, sv = 0.0f;
            for (int j = 0; j < H; ++j) sm = sm + z[l][j];
            const float mean = sm / (float)H;
            for (int j = 0; j < H; ++j) { const float dj = z[l][j] - mean; sv = fmaf(dj, dj, sv); }
            const float rstd = 1.0f / sqrtf(sv / (float)H + 1e-5f);
            if (rstd_out) rstd_out[l] = rstd;
            for (int j = 0; j < H; ++j) {
                const float xn = (z[l][j] - mean) * rstd;
                if (xh) xh[l][j] = xn;
                z[l][j] = fmaf(xn, ln_w[j], ln_b[j]);
            }
        }
        for (int j = 0; j < H; ++j) a[l][j] = act_fwd(d->act, d->prelu, z[l][j]);
        in = a[l];
        n_in = H;
    }
    linear_fwd(p, p + (int64_t)d->out_dim * H, d->out_dim, H, in, y);
}

/* A synthetic env's / reward env's net with `use_layer_norm`: theta holds its nn.Linear parameters only (NES never touches the LayerNorm,
 * GTN_worker.py:156-175), the module keeps weight 1 / bias 0.  Returns a malloc'ed copy of `p` (layout of `plain`) in the layout of the
 * same net with use_layer_norm = 1 -- the two vectors behind the second Linear -- or NULL when there is no position (one hidden layer). */
static float *mlp_with_unit_layer_norm(const orc_mlp_desc *plain, const float *p)
{
    if (plain->layers < 2) return NULL;
    const int64_t H = plain->hidden, head = (int64_t)plain->in_dim * H + H + H * H + H, P = orc_mlp_num_params(plain);
    float *q = malloc(sizeof(float) * (size_t)(P + 2 * H));
    memcpy(q, p, sizeof(float) * (size_t)head);
    for (int64_t j = 0; j < H; ++j) { q[head + j] = 1.0f; q[head + H + j] = 0.0f; }
    memcpy(q + head + 2 * H, p + head, sizeof(float) * (size_t)(P - head));
    return q;
}

static void mlp_forward_one(const orc_mlp_desc *d, const float *p, const float *x, float *y,
                            float z[][ORC_MAX_WIDTH], float a[][ORC_MAX_WIDTH])
{
    mlp_forward_one_ex(d, p, x, y, z, a, NULL, NULL);
}

int orc_mlp_forward(const orc_mlp_desc *d, const float *params, const float *x, int64_t B, float *y, float *hidden_out)
{
    if (d->hidden > ORC_MAX_WIDTH || d->in_dim > ORC_MAX_WIDTH || d->layers > ORC_MAX_LAYERS || d->layers < 1) return -1;
    float (*z)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*a)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    for (int64_t i = 0; i < B; ++i) {
        mlp_forward_one(d, params, x + i * d->in_dim, y + i * d->out_dim, z, a);
        if (hidden_out) memcpy(hidden_out + i * d->hidden, a[d->layers - 1], sizeof(float) * d->hidden);
    }
    free(z); free(a);
    return 0;
}

/* envs/virtual_env.py:43-54 (input = cat(action_onehot, state), three nets on the same input,
 * reward/done see the PRE-transition state) + env_wrapper.py:20-21 (one-hot of the action index)
 * + GTN_worker.py:165-175 (theta +/- eps). */
int orc_se_step_population(const orc_mlp_desc *sn, const orc_mlp_desc *rn, const orc_mlp_desc *dn,
                           const float *theta, const float *eps, const int32_t *worker, const float *sign,
                           int64_t chains, const float *state, const int32_t *action,
                           float *next_state, float *reward, float *done)
{
    const int64_t ps = orc_mlp_num_params(sn), pr = orc_mlp_num_params(rn), pd = orc_mlp_num_params(dn);
    const int64_t P = ps + pr + pd;
    const int S = sn->out_dim, A = sn->in_dim - S;
    if (sn->in_dim > ORC_MAX_WIDTH) return -1;
    float *w = malloc(sizeof(float) * P);
    float x[ORC_MAX_WIDTH];
    for (int64_t c = 0; c < chains; ++c) {
        const float *e = eps ? eps + (int64_t)worker[c] * P : NULL;
        for (int64_t i = 0; i < P; ++i) w[i] = e ? fmaf(sign[c], e[i], theta[i]) : theta[i];
        for (int i = 0; i < A; ++i) x[i] = (i == action[c]) ? 1.0f : 0.0f;
        for (int i = 0; i < S; ++i) x[A + i] = state[c * S + i];
        if (orc_mlp_forward(sn, w, x, 1, next_state + c * S, NULL)) { free(w); return -1; }
        orc_mlp_forward(rn, w + ps, x, 1, reward + c, NULL);
        orc_mlp_forward(dn, w + ps + pr, x, 1, done + c, NULL);
    }
    free(w);
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * real envs -- gym==0.17.3 classic_control (third party, UNPINNED)
 * ---------------------------------------------------------------------------------------- */
void orc_cartpole_step(double st[4], int action, double *reward, int *done)
{
    const double gravity = 9.8, masscart = 1.0, masspole = 0.1, length = 0.5, force_mag = 10.0, tau = 0.02;
    const double total_mass = masspole + masscart;
    const double polemass_length = masspole * length;
    const double theta_thr = 12 * 2 * 3.141592653589793 / 360;
    const double x_thr = 2.4;
    double x = st[0], x_dot = st[1], theta = st[2], theta_dot = st[3];
    double force = action == 1 ? force_mag : -force_mag;
    double costheta = orc_cos(theta), sintheta = orc_sin(theta);
    double temp = (force + polemass_length * (theta_dot * theta_dot) * sintheta) / total_mass;
    double thetaacc = (gravity * sintheta - costheta * temp) /
                      (length * (4.0 / 3.0 - masspole * (costheta * costheta) / total_mass));
    double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    x = x + tau * x_dot;
    x_dot = x_dot + tau * xacc;
    theta = theta + tau * theta_dot;
    theta_dot = theta_dot + tau * thetaacc;
    st[0] = x; st[1] = x_dot; st[2] = theta; st[3] = theta_dot;
    *done = (x < -x_thr || x > x_thr || theta < -theta_thr || theta > theta_thr) ? 1 : 0;
    *reward = 1.0; /* first step past the threshold still pays 1.0; the loop stops on done */
}

/* gym==0.17.3 MountainCar-v0 (classic_control/mountain_car.py; third party, restated): state = (position, velocity) */
void orc_mountaincar_step(double st[4], int action, double *reward, int *done)
{
    double position = st[0], velocity = st[1];
    velocity = velocity + ((double)(action - 1) * 0.001 + orc_cos(3 * position) * (-0.0025));
    velocity = velocity < -0.07 ? -0.07 : (velocity > 0.07 ? 0.07 : velocity);
    position = position + velocity;
    position = position < -1.2 ? -1.2 : (position > 0.6 ? 0.6 : position);
    if (position == -1.2 && velocity < 0) velocity = 0;
    *done = (position >= 0.5 && velocity >= 0) ? 1 : 0;
    *reward = -1.0;
    st[0] = position; st[1] = velocity;
}

void orc_acrobot_step(double st[4], int action, double *reward, int *done);
static void real_env_step(int env_id, double st[4], int action, double *reward, int *done)
{
    if (env_id == ORC_ENV_CARTPOLE) orc_cartpole_step(st, action, reward, done);
    else if (env_id == ORC_ENV_MOUNTAINCAR) orc_mountaincar_step(st, action, reward, done);
    else orc_acrobot_step(st, action, reward, done);
}

static void acrobot_dsdt(const double s[5], double out[5])
{
    const double m1 = 1., m2 = 1., l1 = 1., lc1 = .5, lc2 = .5, I1 = 1., I2 = 1., g = 9.8, pi = 3.141592653589793;
    double a = s[4], theta1 = s[0], theta2 = s[1], dtheta1 = s[2], dtheta2 = s[3];
    double c2 = orc_cos(theta2), s2 = orc_sin(theta2);
    double d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * c2) + I1 + I2;
    double d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
    double phi2 = m2 * lc2 * g * orc_cos(theta1 + theta2 - pi / 2.);
    double phi1 = -m2 * l1 * lc2 * (dtheta2 * dtheta2) * s2 - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * s2 +
                  (m1 * lc1 + m2 * l1) * g * orc_cos(theta1 - pi / 2) + phi2;
    double ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (dtheta1 * dtheta1) * s2 - phi2) /
                      (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1);
    double ddtheta1 = -(d2 * ddtheta2 + phi1) / d1;
    out[0] = dtheta1; out[1] = dtheta2; out[2] = ddtheta1; out[3] = ddtheta2; out[4] = 0.;
}

void orc_acrobot_step(double st[4], int action, double *reward, int *done)
{
    const double pi = 3.141592653589793, dt = .2, dt2 = .2 / 2.0;
    const double max_vel1 = 4 * pi, max_vel2 = 9 * pi;
    double y0[5] = { st[0], st[1], st[2], st[3], (double)(action - 1) };
    double k1[5], k2[5], k3[5], k4[5], tmp[5], ns[5];
    acrobot_dsdt(y0, k1);
    for (int i = 0; i < 5; ++i) tmp[i] = y0[i] + dt2 * k1[i];
    acrobot_dsdt(tmp, k2);
    for (int i = 0; i < 5; ++i) tmp[i] = y0[i] + dt2 * k2[i];
    acrobot_dsdt(tmp, k3);
    for (int i = 0; i < 5; ++i) tmp[i] = y0[i] + dt * k3[i];
    acrobot_dsdt(tmp, k4);
    for (int i = 0; i < 5; ++i) ns[i] = y0[i] + dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    for (int i = 0; i < 2; ++i) {
        double x = ns[i], diff = pi - (-pi);
        while (x > pi) x = x - diff;
        while (x < -pi) x = x + diff;
        ns[i] = x;
    }
    ns[2] = fmin(fmax(ns[2], -max_vel1), max_vel1);
    ns[3] = fmin(fmax(ns[3], -max_vel2), max_vel2);
    for (int i = 0; i < 4; ++i) st[i] = ns[i];
    int terminal = (-orc_cos(st[0]) - orc_cos(st[1] + st[0]) > 1.) ? 1 : 0;
    *done = terminal;
    *reward = terminal ? 0. : -1.;
}

void orc_acrobot_obs(const double st[4], double obs[6])
{
    obs[0] = orc_cos(st[0]); obs[1] = orc_sin(st[0]); obs[2] = orc_cos(st[1]); obs[3] = orc_sin(st[1]);
    obs[4] = st[2]; obs[5] = st[3];
}

/* ------------------------------------------------------------------------------------------
 * DDQN (agents/DDQN.py:60-110)
 * ---------------------------------------------------------------------------------------- */
static inline int argmax_first(const float *v, int n)
{
    int best = 0;
    for (int i = 1; i < n; ++i) if (v[i] > v[best]) best = i;
    return best;
}

/* DDQN.py:79-85: q(s)[a]; a* = argmax online(s'); y = r + gamma*target(s')[a*]*(1-done) */
int orc_qnet_td_forward(const orc_mlp_desc *q, const float *online, const float *target,
                        const float *rows, int64_t row_stride, int64_t B, int32_t S, double gamma,
                        float *q_sa, float *y, int32_t *argmax_next)
{
    if (q->hidden > ORC_MAX_WIDTH || q->layers > ORC_MAX_LAYERS) return -1;
    float (*z)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*a)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float qs[ORC_MAX_WIDTH], qn[ORC_MAX_WIDTH], qt[ORC_MAX_WIDTH];
    const float g32 = (float)gamma;
    for (int64_t b = 0; b < B; ++b) {
        const float *row = rows + b * row_stride;
        const float *s = row, *s2 = row + S + 1;
        int act = (int)row[S];
        float r = row[2 * S + 1], d = row[2 * S + 2];
        mlp_forward_one(q, online, s, qs, z, a);
        mlp_forward_one(q, online, s2, qn, z, a);
        mlp_forward_one(q, target, s2, qt, z, a);
        int am = argmax_first(qn, q->out_dim);
        float t1 = g32 * qt[am];
        float t2 = 1.0f - d;
        float t3 = t1 * t2;
        q_sa[b] = qs[act];
        y[b] = r + t3;
        if (argmax_next) argmax_next[b] = am;
    }
    free(z); free(a);
    return 0;
}

/* One DDQN.learn step (DDQN.py:60-94) on an explicit minibatch `rows` [B, row_stride]:
 * MSE TD loss, backward, torch.optim.Adam single-tensor step, Polyak target update. */
static void mlp_backward_one_ex(const orc_mlp_desc *d, const float *p, const float *x, float z[][ORC_MAX_WIDTH],
                                float a[][ORC_MAX_WIDTH], float xh[][ORC_MAX_WIDTH], const float *rstd, const float *dout,
                                float *g, float *gln, float *dx);
static void mlp_fold_ln_grads(const orc_mlp_desc *d, const float *gln, float *g);

float orc_ddqn_learn(const orc_ddqn_cfg *cfg, float *online, float *target, float *adam_m, float *adam_v,
                     int64_t step, double *b1pow, double *b2pow, const float *rows, int64_t row_stride)
{
    orc_mlp_desc qd = { cfg->state_dim, cfg->q_hidden, cfg->q_layers, cfg->num_actions, cfg->q_act, cfg->q_prelu, cfg->q_layer_norm };
    const int S = cfg->state_dim, H = cfg->q_hidden, L = cfg->q_layers, A = cfg->num_actions, B = cfg->batch_size;
    const int64_t P = orc_mlp_num_params(&qd);
    const int chunk = cfg->grad_chunk > 0 ? cfg->grad_chunk : B;
    float (*z)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*a)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*z2)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*a2)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float *grad = calloc(P, sizeof(float));      /* running sum over finished chunks */
    float *gch = malloc(sizeof(float) * P);      /* current chunk */
    float qs[ORC_MAX_WIDTH], qn[ORC_MAX_WIDTH], qt[ORC_MAX_WIDTH], da[ORC_MAX_WIDTH], dz[ORC_MAX_WIDTH], dprev[ORC_MAX_WIDTH];
    const float g32 = (float)cfg->gamma;
    const float norm = (float)(2.0 / (double)B);   /* mse_loss backward: 2/numel */
    float loss_acc = 0.0f;
    /* use_layer_norm with two or more hidden layers: the generic per-sample backward (LayerNorm positions, shared weight / bias) */
    const int ln = qd.use_layer_norm && L >= 2;
    float (*xh)[ORC_MAX_WIDTH] = ln ? malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH) : NULL;
    float rstd[ORC_MAX_LAYERS];
    float *gln = ln ? malloc(sizeof(float) * (size_t)(L - 1) * 2 * H) : NULL;

    /* layer offsets */
    int64_t offW[ORC_MAX_LAYERS + 1], offb[ORC_MAX_LAYERS + 1];
    {
        int64_t o = 0; int n_in = S;
        for (int l = 0; l < L; ++l) { offW[l] = o; o += (int64_t)H * n_in; offb[l] = o; o += H; n_in = H; }
        offW[L] = o; o += (int64_t)A * H; offb[L] = o;
    }

    int first_chunk = 1;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        int b1 = b0 + chunk < B ? b0 + chunk : B;
        memset(gch, 0, sizeof(float) * P);
        if (ln) memset(gln, 0, sizeof(float) * (size_t)(L - 1) * 2 * H);
        for (int b = b0; b < b1; ++b) {
            const float *row = rows + (int64_t)b * row_stride;
            const float *s = row, *s2 = row + S + 1;
            int act = (int)row[S];
            float r = row[2 * S + 1], d = row[2 * S + 2];
            mlp_forward_one(&qd, online, s2, qn, z2, a2);
            mlp_forward_one(&qd, target, s2, qt, z2, a2);
            mlp_forward_one_ex(&qd, online, s, qs, z, a, xh, ln ? rstd : NULL);
            int am = argmax_first(qn, A);
            float t1 = g32 * qt[am];
            float t2 = 1.0f - d;
            float yv = r + t1 * t2;
            float diff = qs[act] - yv;
            loss_acc = fmaf(diff, diff, loss_acc);
            float dq = norm * diff;
            if (ln) {
                float dout[ORC_MAX_WIDTH];
                for (int o = 0; o < A; ++o) dout[o] = o == act ? dq : 0.0f;
                mlp_backward_one_ex(&qd, online, s, z, a, xh, rstd, dout, gch, gln, NULL);
                continue;
            }
            /* output layer: only row `act` of dQ is non-zero */
            {
                float *gW = gch + offW[L] + (int64_t)act * H;
                const float *W = online + offW[L] + (int64_t)act * H;
                for (int j = 0; j < H; ++j) {
                    gW[j] = fmaf(dq, a[L - 1][j], gW[j]);
                    da[j] = dq * W[j];
                }
                gch[offb[L] + act] = gch[offb[L] + act] + dq;
            }
            for (int l = L - 1; l >= 0; --l) {
                int n_in = l == 0 ? S : H;
                const float *inp = l == 0 ? s : a[l - 1];
                for (int j = 0; j < H; ++j) dz[j] = act_bwd(cfg->q_act, cfg->q_prelu, z[l][j], a[l][j], da[j]);
                float *gW = gch + offW[l];
                float *gb = gch + offb[l];
                for (int j = 0; j < H; ++j) {
                    for (int i = 0; i < n_in; ++i) gW[(int64_t)j * n_in + i] = fmaf(dz[j], inp[i], gW[(int64_t)j * n_in + i]);
                    gb[j] = gb[j] + dz[j];
                }
                if (l > 0) {
                    const float *W = online + offW[l];
                    for (int i = 0; i < n_in; ++i) {
                        float acc = 0.0f;
                        for (int j = 0; j < H; ++j) acc = fmaf(dz[j], W[(int64_t)j * n_in + i], acc);
                        dprev[i] = acc;
                    }
                    memcpy(da, dprev, sizeof(float) * n_in);
                }
            }
        }
        if (ln) mlp_fold_ln_grads(&qd, gln, gch);
        if (first_chunk) { memcpy(grad, gch, sizeof(float) * P); first_chunk = 0; }
        else for (int64_t i = 0; i < P; ++i) grad[i] = grad[i] + gch[i];
    }

    /* torch.optim.Adam (_single_tensor_adam), weight_decay 0, amsgrad False */
    *b1pow *= cfg->adam_beta1;
    *b2pow *= cfg->adam_beta2;
    (void)step;
    const double bc1 = 1.0 - *b1pow, bc2 = 1.0 - *b2pow;
    const float neg_step = (float)(-(cfg->lr / bc1));
    const float bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - cfg->adam_beta1), w2 = (float)(1.0 - cfg->adam_beta2);
    const float beta2 = (float)cfg->adam_beta2, eps = (float)cfg->adam_eps;
    const float tau = (float)cfg->tau, omt = (float)(1.0 - cfg->tau);
    for (int64_t i = 0; i < P; ++i) {
        float g = grad[i];
        float m = fmaf(w1, g - adam_m[i], adam_m[i]);            /* exp_avg.lerp_(grad, 1-beta1) */
        float v = adam_v[i] * beta2;                              /* exp_avg_sq.mul_(beta2) */
        v = fmaf(w2 * g, g, v);                                   /* .addcmul_(grad, grad, value=1-beta2) */
        float denom = sqrtf(v) / bc2_sqrt + eps;
        float p = online[i] + (neg_step * m) / denom;             /* param.addcdiv_(exp_avg, denom, value=-step_size) */
        adam_m[i] = m; adam_v[i] = v; online[i] = p;
        target[i] = tau * p + omt * target[i];                    /* DDQN.py:92-93 */
    }
    free(z); free(a); free(z2); free(a2); free(grad); free(gch); free(xh); free(gln);
    return loss_acc / (float)B;
}

/* ------------------------------------------------------------------------------------------
 * DuelingDDQN (agents/DuelingDDQN.py:59-110, models/actor_critic.py:94-122)
 * ---------------------------------------------------------------------------------------- */
typedef struct { orc_mlp_desc feat, val, adv; int64_t p_feat, p_val, p_adv, P; } dueling_layout;

static void dueling_layout_of(const orc_ddqn_cfg *cfg, dueling_layout *L)
{
    const int F = cfg->feature_dim;
    L->feat = (orc_mlp_desc){ cfg->state_dim, cfg->q_hidden, cfg->q_layers, F, cfg->q_act, cfg->q_prelu, cfg->q_layer_norm };
    /* heads_config: hidden_layer = 1, hidden_size = feature_dim (actor_critic.py:103-105) */
    L->val = (orc_mlp_desc){ F, F, 1, 1, cfg->q_act, cfg->q_prelu, 0 };
    L->adv = (orc_mlp_desc){ F, F, 1, cfg->num_actions, cfg->q_act, cfg->q_prelu, 0 };
    L->p_feat = orc_mlp_num_params(&L->feat);
    L->p_val = orc_mlp_num_params(&L->val);
    L->p_adv = orc_mlp_num_params(&L->adv);
    L->P = L->p_feat + L->p_val + L->p_adv;
}

int64_t orc_dueling_num_params(const orc_ddqn_cfg *cfg)
{
    dueling_layout L;
    dueling_layout_of(cfg, &L);
    return L.P;
}

/* per-sample scratch of one dueling forward */
typedef struct {
    float zf[ORC_MAX_LAYERS][ORC_MAX_WIDTH], af[ORC_MAX_LAYERS][ORC_MAX_WIDTH];
    float xhf[ORC_MAX_LAYERS][ORC_MAX_WIDTH], rstdf[ORC_MAX_LAYERS];      /* the feature stream's LayerNorm positions (q_layer_norm) */
    float zv[1][ORC_MAX_WIDTH], av[1][ORC_MAX_WIDTH], za[1][ORC_MAX_WIDTH], aa[1][ORC_MAX_WIDTH];
    float feat[ORC_MAX_WIDTH], V, adv[64];
} dueling_act;

static void dueling_forward_one(const dueling_layout *L, const float *p, const float *x, dueling_act *s)
{
    mlp_forward_one_ex(&L->feat, p, x, s->feat, s->zf, s->af, s->xhf, s->rstdf);  /* no activation after the last Linear */
    mlp_forward_one(&L->val, p + L->p_feat, s->feat, &s->V, s->zv, s->av);
    mlp_forward_one(&L->adv, p + L->p_feat + L->p_val, s->feat, s->adv, s->za, s->aa);
}

/* q = values + (advantages - advantages.mean()); the mean runs over every element of the [B,A] tensor
 * (actor_critic.py:121), summed sequentially in row-major order here */
int orc_dueling_forward(const orc_ddqn_cfg *cfg, const float *params, const float *x, int64_t B, float *q)
{
    dueling_layout L;
    dueling_layout_of(cfg, &L);
    if (cfg->feature_dim > ORC_MAX_WIDTH || cfg->q_hidden > ORC_MAX_WIDTH || cfg->num_actions > 64 || cfg->q_layers > ORC_MAX_LAYERS) return -1;
    const int A = cfg->num_actions;
    dueling_act *s = malloc(sizeof(dueling_act));
    float *V = malloc(sizeof(float) * B), *adv = malloc(sizeof(float) * B * A);
    float sum = 0.0f;
    for (int64_t b = 0; b < B; ++b) {
        dueling_forward_one(&L, params, x + b * cfg->state_dim, s);
        V[b] = s->V;
        for (int a = 0; a < A; ++a) { adv[b * A + a] = s->adv[a]; sum = sum + s->adv[a]; }
    }
    const float mean = sum / (float)(B * A);
    for (int64_t b = 0; b < B; ++b)
        for (int a = 0; a < A; ++a) q[b * A + a] = V[b] + (adv[b * A + a] - mean);
    free(s); free(V); free(adv);
    return 0;
}

/* backward of one MLP for one sample: accumulates parameter gradients into g (same layout as p), returns dL/dx */
static void mlp_backward_one_ex(const orc_mlp_desc *d, const float *p, const float *x, float z[][ORC_MAX_WIDTH],
                                float a[][ORC_MAX_WIDTH], float xh[][ORC_MAX_WIDTH], const float *rstd, const float *dout,
                                float *g, float *gln, float *dx)
{
    const int H = d->hidden, L = d->layers, O = d->out_dim;
    const int ln = d->use_layer_norm && L >= 2;
    int64_t offW[ORC_MAX_LAYERS + 1], offb[ORC_MAX_LAYERS + 1], off_ln = 0;
    {
        int64_t o = 0; int n_in = d->in_dim;
        for (int l = 0; l < L; ++l) {
            offW[l] = o; o += (int64_t)H * n_in; offb[l] = o; o += H; n_in = H;
            if (ln && l == 1) { off_ln = o; o += 2 * H; }         /* the shared nn.LayerNorm sits behind the second Linear */
        }
        offW[L] = o; o += (int64_t)O * H; offb[L] = o;
    }
    float da[ORC_MAX_WIDTH], dz[ORC_MAX_WIDTH], dprev[ORC_MAX_WIDTH];
    for (int o = 0; o < O; ++o) {
        float *gW = g + offW[L] + (int64_t)o * H;
        for (int j = 0; j < H; ++j) gW[j] = fmaf(dout[o], a[L - 1][j], gW[j]);
        g[offb[L] + o] = g[offb[L] + o] + dout[o];
    }
    for (int j = 0; j < H; ++j) {
        float acc = 0.0f;
        for (int o = 0; o < O; ++o) acc = fmaf(dout[o], p[offW[L] + (int64_t)o * H + j], acc);
        da[j] = acc;
    }
    for (int l = L - 1; l >= 0; --l) {
        const int n_in = l == 0 ? d->in_dim : H;
        const float *inp = l == 0 ? x : a[l - 1];
        for (int j = 0; j < H; ++j) dz[j] = act_bwd(d->act, d->prelu, z[l][j], a[l][j], da[j]);
        if (ln && l >= 1) {
            /* LayerNorm backward.  dz = grad of the LayerNorm output; its weight / bias gradients accumulate per POSITION
             * (gln [(L-1)][2][H], position l - 1; the caller adds the positions up, last layer first); the input gradient
             * is rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)) with sequential sums */
            float *gw = gln + (int64_t)(l - 1) * 2 * H, *gb = gw + H;
            const float *w = p + off_ln;
            float s1 = 0.0f, s2 = 0.0f;
            for (int j = 0; j < H; ++j) {
                gw[j] = fmaf(dz[j], xh[l][j], gw[j]);
                gb[j] = gb[j] + dz[j];
                dz[j] = dz[j] * w[j];
            }
            for (int j = 0; j < H; ++j) s1 = s1 + dz[j];
            for (int j = 0; j < H; ++j) s2 = fmaf(dz[j], xh[l][j], s2);
            const float m1 = s1 / (float)H, m2 = s2 / (float)H;
            for (int j = 0; j < H; ++j) dz[j] = fmaf(-xh[l][j], m2, dz[j] - m1) * rstd[l];
        }
        float *gW = g + offW[l], *gb = g + offb[l];
        for (int j = 0; j < H; ++j) {
            for (int i = 0; i < n_in; ++i) gW[(int64_t)j * n_in + i] = fmaf(dz[j], inp[i], gW[(int64_t)j * n_in + i]);
            gb[j] = gb[j] + dz[j];
        }
        if (l > 0 || dx) {
            const float *W = p + offW[l];
            for (int i = 0; i < n_in; ++i) {
                float acc = 0.0f;
                for (int j = 0; j < H; ++j) acc = fmaf(dz[j], W[(int64_t)j * n_in + i], acc);
                dprev[i] = acc;
            }
            if (l > 0) memcpy(da, dprev, sizeof(float) * n_in);
            else memcpy(dx, dprev, sizeof(float) * n_in);
        }
    }
}

/* fold the per-position LayerNorm gradients of mlp_backward_one_ex into the flat gradient: position L-1 first, then down */
static void mlp_fold_ln_grads(const orc_mlp_desc *d, const float *gln, float *g)
{
    const int H = d->hidden, L = d->layers;
    if (!(d->use_layer_norm && L >= 2)) return;
    float *gl = g + (int64_t)d->in_dim * H + H + (int64_t)H * H + H;
    for (int j = 0; j < 2 * H; ++j) {
        float acc = gln[(int64_t)(L - 2) * 2 * H + j];
        for (int pos = L - 3; pos >= 0; --pos) acc = acc + gln[(int64_t)pos * 2 * H + j];
        gl[j] = acc;
    }
}

static void mlp_backward_one(const orc_mlp_desc *d, const float *p, const float *x, float z[][ORC_MAX_WIDTH],
                             float a[][ORC_MAX_WIDTH], const float *dout, float *g, float *dx)
{
    mlp_backward_one_ex(d, p, x, z, a, NULL, NULL, dout, g, NULL, dx);      /* plain MLPs only (use_layer_norm == 0) */
}

/* One DuelingDDQN.learn step (DuelingDDQN.py:59-94): forward of the three batches with the GLOBAL advantage mean,
 * loss = mse_loss(expected.detach(), q_value), backward through the mean, Adam, Polyak. */
float orc_dueling_learn(const orc_ddqn_cfg *cfg, float *online, float *target, float *adam_m, float *adam_v,
                        double *b1pow, double *b2pow, const float *rows, int64_t row_stride)
{
    dueling_layout L;
    dueling_layout_of(cfg, &L);
    const int S = cfg->state_dim, A = cfg->num_actions, B = cfg->batch_size, F = cfg->feature_dim;
    const int64_t P = L.P;
    const int chunk = cfg->grad_chunk > 0 ? cfg->grad_chunk : B;
    dueling_act *acts = malloc(sizeof(dueling_act) * (size_t)B);      /* online(s) activations of every sample */
    float *s_in = malloc(sizeof(float) * (size_t)B * S), *s2_in = malloc(sizeof(float) * (size_t)B * S);
    float *q = malloc(sizeof(float) * (size_t)B * A), *qn = malloc(sizeof(float) * (size_t)B * A), *qt = malloc(sizeof(float) * (size_t)B * A);
    float *dq = malloc(sizeof(float) * (size_t)B);
    float *grad = calloc(P, sizeof(float)), *gch = malloc(sizeof(float) * P);
    for (int b = 0; b < B; ++b) {
        memcpy(s_in + (size_t)b * S, rows + (int64_t)b * row_stride, sizeof(float) * S);
        memcpy(s2_in + (size_t)b * S, rows + (int64_t)b * row_stride + S + 1, sizeof(float) * S);
    }
    /* q_values = model(states) keeping the activations */
    {
        float sum = 0.0f;
        for (int b = 0; b < B; ++b) {
            dueling_forward_one(&L, online, s_in + (size_t)b * S, &acts[b]);
            for (int a = 0; a < A; ++a) sum = sum + acts[b].adv[a];
        }
        const float mean = sum / (float)(B * A);
        for (int b = 0; b < B; ++b)
            for (int a = 0; a < A; ++a) q[b * A + a] = acts[b].V + (acts[b].adv[a] - mean);
    }
    orc_dueling_forward(cfg, online, s2_in, B, qn);
    orc_dueling_forward(cfg, target, s2_in, B, qt);
    const float g32 = (float)cfg->gamma, norm = (float)(2.0 / (double)B);
    float loss_acc = 0.0f, S_dq = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float *row = rows + (int64_t)b * row_stride;
        const int act = (int)row[S];
        const float r = row[2 * S + 1], d = row[2 * S + 2];
        const int am = argmax_first(qn + b * A, A);
        const float t1 = g32 * qt[b * A + am];
        const float t2 = 1.0f - d;
        const float yv = r + t1 * t2;
        const float diff = q[b * A + act] - yv;
        loss_acc = fmaf(diff, diff, loss_acc);
        dq[b] = norm * diff;
        S_dq = S_dq + dq[b];                       /* sum of dL/dQ over the whole [B,A] tensor (one non-zero per row) */
    }
    const float mean_grad = (-S_dq) / (float)(B * A);   /* backward of `- advantages.mean()` */
    int first_chunk = 1;
    float dadv[64], dfeat_v[ORC_MAX_WIDTH], dfeat_a[ORC_MAX_WIDTH], dfeat[ORC_MAX_WIDTH];
    const int ln = L.feat.use_layer_norm && L.feat.layers >= 2;
    const size_t gln_n = ln ? (size_t)(L.feat.layers - 1) * 2 * L.feat.hidden : 0;
    float *gln = ln ? malloc(sizeof(float) * gln_n) : NULL;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int b1 = b0 + chunk < B ? b0 + chunk : B;
        memset(gch, 0, sizeof(float) * P);
        if (ln) memset(gln, 0, sizeof(float) * gln_n);
        for (int b = b0; b < b1; ++b) {
            const int act = (int)rows[(int64_t)b * row_stride + S];
            for (int a = 0; a < A; ++a) dadv[a] = (a == act ? dq[b] : 0.0f) + mean_grad;
            const float dV = dq[b];
            mlp_backward_one(&L.val, online + L.p_feat, acts[b].feat, acts[b].zv, acts[b].av, &dV, gch + L.p_feat, dfeat_v);
            mlp_backward_one(&L.adv, online + L.p_feat + L.p_val, acts[b].feat, acts[b].za, acts[b].aa, dadv,
                             gch + L.p_feat + L.p_val, dfeat_a);
            for (int i = 0; i < F; ++i) dfeat[i] = dfeat_v[i] + dfeat_a[i];
            mlp_backward_one_ex(&L.feat, online, s_in + (size_t)b * S, acts[b].zf, acts[b].af, acts[b].xhf, acts[b].rstdf, dfeat, gch, gln, NULL);
        }
        if (ln) mlp_fold_ln_grads(&L.feat, gln, gch);
        if (first_chunk) { memcpy(grad, gch, sizeof(float) * P); first_chunk = 0; }
        else for (int64_t i = 0; i < P; ++i) grad[i] = grad[i] + gch[i];
    }
    *b1pow *= cfg->adam_beta1;
    *b2pow *= cfg->adam_beta2;
    const double bc1 = 1.0 - *b1pow, bc2 = 1.0 - *b2pow;
    const float neg_step = (float)(-(cfg->lr / bc1));
    const float bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - cfg->adam_beta1), w2 = (float)(1.0 - cfg->adam_beta2);
    const float beta2 = (float)cfg->adam_beta2, eps = (float)cfg->adam_eps;
    const float tau = (float)cfg->tau, omt = (float)(1.0 - cfg->tau);
    for (int64_t i = 0; i < P; ++i) {
        const float g = grad[i];
        const float m = fmaf(w1, g - adam_m[i], adam_m[i]);
        float v = adam_v[i] * beta2;
        v = fmaf(w2 * g, g, v);
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        const float pnew = online[i] + (neg_step * m) / denom;
        adam_m[i] = m; adam_v[i] = v; online[i] = pnew;
        target[i] = tau * pnew + omt * target[i];
    }
    free(acts); free(s_in); free(s2_in); free(q); free(qn); free(qt); free(dq); free(grad); free(gch); free(gln);
    return loss_acc / (float)B;
}

/* agent dispatch used by the chain: greedy action and learn step of the configured inner agent */
static int64_t agent_num_params(const orc_ddqn_cfg *cfg)
{
    if (cfg->agent_kind == 1) return orc_dueling_num_params(cfg);
    orc_mlp_desc qd = { cfg->state_dim, cfg->q_hidden, cfg->q_layers, cfg->num_actions, cfg->q_act, cfg->q_prelu, cfg->q_layer_norm };
    return orc_mlp_num_params(&qd);
}

static int agent_greedy_action(const orc_ddqn_cfg *cfg, const float *params, const float *obs,
                               float (*z)[ORC_MAX_WIDTH], float (*a)[ORC_MAX_WIDTH])
{
    float q[ORC_MAX_WIDTH];
    if (cfg->agent_kind == 1) {
        orc_dueling_forward(cfg, params, obs, 1, q);       /* single state: the mean is over its A advantages */
    } else {
        orc_mlp_desc qd = { cfg->state_dim, cfg->q_hidden, cfg->q_layers, cfg->num_actions, cfg->q_act, cfg->q_prelu, cfg->q_layer_norm };
        mlp_forward_one(&qd, params, obs, q, z, a);
    }
    return argmax_first(q, cfg->num_actions);
}

/* ------------------------------------------------------------------------------------------
 * One chain: GTN_Worker.calc_score (GTN_worker.py:187-221) =
 *   select_agent -> DDQN (fresh agent, agent_init weights) ; BaseAgent.train(env=SE, test_env=real)
 *   (base_agent.py:64-153) ; BaseAgent.test(real) (base_agent.py:155-227) ; statistics.mean.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const orc_ddqn_cfg *cfg;
    uint64_t key;
    const orc_tapes *tapes;
    int64_t n_eps, n_act, n_test_ep, n_train_ep;
    int err;
} rng_state;

static double draw_eps_uniform(rng_state *r)
{
    int64_t n = r->n_eps++;
    if (r->cfg->rng_mode == ORC_RNG_TAPE) {
        if (n >= r->tapes->n_eps_uniform) { r->err = -2; return 1.0; }
        return r->tapes->eps_uniform[n];
    }
    return u64_to_unit(orc_rng_u64(r->key, STREAM_EPS, (uint64_t)n));
}

static int draw_rand_action(rng_state *r)
{
    int64_t n = r->n_act++;
    if (r->cfg->rng_mode == ORC_RNG_TAPE) {
        if (n >= r->tapes->n_rand_action) { r->err = -3; return 0; }
        return r->tapes->rand_action[n];
    }
    return (int)u64_to_below(orc_rng_u64(r->key, STREAM_ACTION, (uint64_t)n), (uint32_t)r->cfg->num_actions);
}

static int draw_replay_idx(rng_state *r, int64_t learn_it, int b, int64_t size)
{
    int64_t n = learn_it * r->cfg->batch_size + b;
    if (r->cfg->rng_mode == ORC_RNG_TAPE) {
        if (n >= r->tapes->n_replay_idx) { r->err = -4; return 0; }
        return r->tapes->replay_idx[n];
    }
    return (int)orc_rng_replay_below(r->key, (uint64_t)n, (uint32_t)size);
}

/* gym reset: np_random.uniform(low, high, size=(4,)) = low + (high-low)*u */
static void draw_reset(rng_state *r, int train, int64_t ep, double st[4])
{
    const double lim = r->cfg->env_id == ORC_ENV_CARTPOLE ? 0.05 : 0.1;
    if (r->cfg->rng_mode != ORC_RNG_TAPE && r->cfg->env_id == ORC_ENV_MOUNTAINCAR) {
        /* mountain_car.py reset: position ~ U(-0.6, -0.4), velocity 0 */
        st[0] = -0.6 + 0.2 * u64_to_unit(orc_rng_u64(r->key, train ? STREAM_TRAIN_RESET : STREAM_TEST_RESET, (uint64_t)(ep * 4)));
        st[1] = st[2] = st[3] = 0.0;
        return;
    }
    if (r->cfg->rng_mode == ORC_RNG_TAPE) {
        const double *tp = train ? r->tapes->train_reset : r->tapes->test_reset;
        int64_t nrows = train ? r->tapes->n_train_reset : r->tapes->n_test_reset;
        if (ep >= nrows) { r->err = -5; memset(st, 0, sizeof(double) * 4); return; }
        memcpy(st, tp + ep * 4, sizeof(double) * 4);
        return;
    }
    for (int i = 0; i < 4; ++i) {
        double u = u64_to_unit(orc_rng_u64(r->key, train ? STREAM_TRAIN_RESET : STREAM_TEST_RESET, (uint64_t)(ep * 4 + i)));
        st[i] = -lim + (2 * lim) * u;
    }
}

static void real_env_obs(int env_id, const double st[4], float *obs)
{
    if (env_id == ORC_ENV_CARTPOLE) {
        for (int i = 0; i < 4; ++i) obs[i] = (float)st[i];
    } else if (env_id == ORC_ENV_MOUNTAINCAR) {
        obs[0] = (float)st[0]; obs[1] = (float)st[1];
    } else {
        double o[6];
        orc_acrobot_obs(st, o);
        for (int i = 0; i < 6; ++i) obs[i] = (float)o[i];
    }
}

/* BaseAgent.test (base_agent.py:155-227) with DDQN.select_test_action (DDQN.py:106-110): greedy. */
static void run_test_phase(const orc_ddqn_cfg *cfg, const orc_mlp_desc *qd, const float *online, rng_state *rng,
                           double *returns, int64_t *test_steps, float (*z)[ORC_MAX_WIDTH], float (*a)[ORC_MAX_WIDTH])
{
    float obs[8];
    (void)qd;
    for (int te = 0; te < cfg->test_episodes; ++te) {
        double st[4];
        draw_reset(rng, 0, rng->n_test_ep++, st);
        float ep_reward = 0.0f;   /* fp32 tensor accumulation, base_agent.py:212 */
        const int k_rep = cfg->same_action_num > 1 ? cfg->same_action_num : 1;
        int env_steps = 0, done = 0;
        for (int t = 0; t < cfg->max_steps && !done; t += k_rep) {       /* base_agent.py:194 range(0, max_steps, same_action_num) */
            real_env_obs(cfg->env_id, st, obs);
            int act = agent_greedy_action(cfg, online, obs, z, a);
            /* EnvWrapper.step on a real env (env_wrapper.py:56-61): reward_sum = 0; += reward; break on done (TimeLimit: elapsed >=
             * max_steps -> done) */
            double rsum = 0.0;
            for (int r_ = 0; r_ < k_rep; ++r_) {
                double rew;
                real_env_step(cfg->env_id, st, act, &rew, &done);
                rsum = rsum + rew;
                ++*test_steps; ++env_steps;
                if (env_steps >= cfg->max_steps) done = 1;
                if (done) break;
            }
            ep_reward = ep_reward + (float)rsum;
        }
        returns[te] = (double)ep_reward;
    }
}

/* BaseAgent.test under a time-out (base_agent.py:177-184 + time_is_up :30-47) with the env-step budget standing in for
 * wall-clock: episode e starts only while the steps of this test's earlier episodes do not exceed `remaining`; from the
 * first episode that may not start, the returns are padded with the minimum so far (-1e9 if there is none).  The episodes
 * are independent, so all of them are rolled out and the list is cut afterwards; *test_steps counts the ones that ran. */
static void run_test_phase_budget(const orc_ddqn_cfg *cfg, const orc_mlp_desc *qd, const float *online, rng_state *rng,
                                  double *returns, int64_t *test_steps, float (*z)[ORC_MAX_WIDTH], float (*a)[ORC_MAX_WIDTH],
                                  int64_t remaining)
{
    int64_t used = 0;
    int stop = cfg->test_episodes;
    int64_t *len = malloc(sizeof(int64_t) * (cfg->test_episodes > 0 ? cfg->test_episodes : 1));
    for (int te = 0; te < cfg->test_episodes; ++te) {
        int64_t steps = 0;
        double r1;
        /* one episode at a time through the ordinary phase code (test_episodes = 1 view) */
        orc_ddqn_cfg one = *cfg; one.test_episodes = 1;
        run_test_phase(&one, qd, online, rng, &r1, &steps, z, a);
        returns[te] = r1; len[te] = steps;
    }
    for (int te = 0; te < cfg->test_episodes; ++te) {
        if (used > remaining) { stop = te; break; }
        used += len[te];
    }
    for (int te = stop; te < cfg->test_episodes; ++te) {
        double mn = -1e9;
        if (stop > 0) { mn = returns[0]; for (int i = 1; i < stop; ++i) if (returns[i] < mn) mn = returns[i]; }
        returns[te] = mn;
    }
    *test_steps += used;
    free(len);
}

/* time_is_up for a finished test phase (base_agent.py:177-184 + :30-47) with per-episode lengths: episode e may start only
 * while the earlier episodes used <= remaining steps; later returns are padded with the minimum so far (-1e9 if none).
 * Returns the steps of the episodes that ran. */
static int64_t budget_cut_test(double *returns, const int64_t *len, int T, int64_t remaining)
{
    int64_t used = 0;
    int stop = T;
    for (int te = 0; te < T; ++te) {
        if (used > remaining) { stop = te; break; }
        used += len[te];
    }
    double mn = -1e9;
    if (stop > 0) { mn = returns[0]; for (int i = 1; i < stop; ++i) if (returns[i] < mn) mn = returns[i]; }
    for (int te = stop; te < T; ++te) returns[te] = mn;
    return used;
}

/* time_is_up padding of the per-episode lists after a training time-out (base_agent.py:33-44) */
static void budget_pad_train(double *episode_test_mean, int32_t *episode_len, const double *meter, int n_meter, int episodes_run, int train_episodes)
{
    double mn = -1e9; int mx = 1000000000;
    if (n_meter > 0) { mn = meter[0]; for (int i = 1; i < n_meter; ++i) if (meter[i] < mn) mn = meter[i]; }
    if (episodes_run > 0 && episode_len) { mx = episode_len[0]; for (int i = 1; i < episodes_run; ++i) if (episode_len[i] > mx) mx = episode_len[i]; }
    for (int e = episodes_run; e < train_episodes; ++e) {
        if (episode_test_mean) episode_test_mean[e] = mn;
        if (episode_len) episode_len[e] = mx;
    }
}

/* BaseAgent.env_solved (base_agent.py:49-62) over the reward meter's list (AverageMeter.get_mean / get_mean_last / _mean,
 * utils.py:94-105: a slice sum over (len + 1e-9)); called for episode >= init_episodes only (base_agent.py:141).
 * virtual_rule: break_env is a VirtualEnv (train(env, test_env=None) on one) -- relative change of the last `num` entries' mean
 * against the `num` before them; otherwise the real rule avg >= solved_reward. */
static int meter_env_solved(const double *meter, int n, int num, int virtual_rule, double solved_reward, double virtual_diff, int episode,
                            int init_episodes)
{
    int lo = n - num; if (lo < 0) lo = 0;
    double sm = 0.0;
    for (int i = lo; i < n; ++i) sm += meter[i];
    const double avg = sm / ((double)(n - lo) + 1e-9);
    if (!virtual_rule) return avg >= solved_reward;
    int hi2 = n - num; if (hi2 < 0) hi2 = 0;
    int lo2 = n - 2 * num; if (lo2 < 0) lo2 = 0;
    double s2 = 0.0;
    for (int i = lo2; i < hi2; ++i) s2 += meter[i];
    const double last = s2 / ((double)(hi2 - lo2) + 1e-9);
    return fabs(avg - last) / (fabs(last) + 1e-9) < virtual_diff && episode >= init_episodes + num;
}

static double mean_seq(const double *v, int n)
{
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += v[i];
    return s / (double)n;
}

#include "lenv_oracle_icm.inc"

/* RewardEnv._calc_reward for one transition (defined with the TD3 / RewardEnv code in lenv_oracle_td3.inc) */
static float rn_shape_one(int t, int S, int info_dim, const orc_mlp_desc *rd, const float *rn_params, float g32, const float *state,
                          const float *next_state, const float *info, float r32, float *phi_s_cache, int have_cache,
                          float (*z)[ORC_MAX_WIDTH], float (*a)[ORC_MAX_WIDTH]);

static int ddqn_se_chain_impl(const orc_ddqn_cfg *cfg, const float *se_params, const float *agent_init, const float *icm_init, uint64_t rng_key,
                              const orc_tapes *tapes, double *episode_test_mean, int32_t *episode_len,
                              double *final_test_returns, orc_trace *trace, orc_chain_result *res, float *icm_final, float *final_online);

int orc_ddqn_se_chain_icm(const orc_ddqn_cfg *cfg, const float *se_params, const float *agent_init, const float *icm_init, uint64_t rng_key,
                          const orc_tapes *tapes, double *episode_test_mean, int32_t *episode_len,
                          double *final_test_returns, orc_trace *trace, orc_chain_result *res, float *icm_final)
{
    return ddqn_se_chain_impl(cfg, se_params, agent_init, icm_init, rng_key, tapes, episode_test_mean, episode_len, final_test_returns, trace, res,
                              icm_final, NULL);
}

/* the same, also handing out the trained online net (flat state-dict order, orc_mlp_num_params / orc_dueling_num_params floats) */
int orc_ddqn_se_chain_params(const orc_ddqn_cfg *cfg, const float *se_params, const float *agent_init, uint64_t rng_key,
                             const orc_tapes *tapes, double *episode_test_mean, int32_t *episode_len,
                             double *final_test_returns, orc_trace *trace, orc_chain_result *res, float *final_online)
{
    if (cfg->icm_enabled) return -1;
    return ddqn_se_chain_impl(cfg, se_params, agent_init, NULL, rng_key, tapes, episode_test_mean, episode_len, final_test_returns, trace, res,
                              NULL, final_online);
}

int orc_ddqn_se_chain(const orc_ddqn_cfg *cfg, const float *se_params, const float *agent_init, uint64_t rng_key,
                      const orc_tapes *tapes, double *episode_test_mean, int32_t *episode_len,
                      double *final_test_returns, orc_trace *trace, orc_chain_result *res)
{
    if (cfg->icm_enabled) return -1;               /* an ICM agent needs its own fresh ICM parameters: orc_ddqn_se_chain_icm */
    return orc_ddqn_se_chain_icm(cfg, se_params, agent_init, NULL, rng_key, tapes, episode_test_mean, episode_len, final_test_returns,
                                 trace, res, NULL);
}

/* icm_init: [orc_icm_num_params] fresh ICMModel parameters in state-dict order when cfg->icm_enabled, else NULL;
 * icm_final (may be NULL): the ICM parameters after the last learn step */
static int ddqn_se_chain_impl(const orc_ddqn_cfg *cfg, const float *se_params, const float *agent_init, const float *icm_init, uint64_t rng_key,
                              const orc_tapes *tapes, double *episode_test_mean, int32_t *episode_len,
                              double *final_test_returns, orc_trace *trace, orc_chain_result *res, float *icm_final, float *final_online)
{
    const int S = cfg->state_dim, A = cfg->num_actions, B = cfg->batch_size;
    if (cfg->icm_enabled && !icm_init) return -1;
    icm_net icm;
    icm_hp ihp = { cfg->icm_lr, cfg->icm_beta, cfg->icm_eta, cfg->adam_beta1, cfg->adam_beta2, cfg->adam_eps };
    float *icm_p = NULL, *icm_m = NULL, *icm_v = NULL, *r_intr = NULL;
    double icm_pows[2] = { 1.0, 1.0 };
    if (cfg->icm_enabled) {
        icm_build(&icm, S, A, cfg->icm_feature_dim, cfg->icm_hidden, 1);
        icm_p = malloc(sizeof(float) * icm.P); icm_m = calloc(icm.P, sizeof(float)); icm_v = calloc(icm.P, sizeof(float));
        r_intr = malloc(sizeof(float) * B);
        memcpy(icm_p, icm_init, sizeof(float) * icm.P);
    }
    orc_mlp_desc qd = { S, cfg->q_hidden, cfg->q_layers, A, cfg->q_act, cfg->q_prelu, cfg->q_layer_norm };
    orc_mlp_desc sn = { S + A, cfg->se_hidden, cfg->se_layers, S, cfg->se_act, cfg->se_prelu, 0 };
    orc_mlp_desc rn = sn, dn = sn;
    rn.out_dim = 1; dn.out_dim = 1;
    if (cfg->env_id == ORC_ENV_CARTPOLE && S != 4) return -1;
    if (cfg->env_id == ORC_ENV_ACROBOT && S != 6) return -1;
    if (cfg->env_id == ORC_ENV_MOUNTAINCAR && (S != 2 || A != 3)) return -1;
    if (cfg->q_hidden > ORC_MAX_WIDTH || cfg->se_hidden > ORC_MAX_WIDTH || S + A > 64) return -1;
    if (cfg->rng_mode == ORC_RNG_TAPE && !tapes) return -1;
    const int reward_env = cfg->synthetic_env_type == 1;
    const int rtype = cfg->reward_env_type;
    if (reward_env && !(rtype == 0 || rtype == 1 || rtype == 2 || rtype == 5 || rtype == 6)) return -1;   /* info types: no info vector here */
    /* RewardEnv.build_reward_net (reward_env.py:29-46): an MLP on the state (a 1-input dummy for type 0) */
    orc_mlp_desc rd = { rtype == 0 ? 1 : S, cfg->se_hidden, cfg->se_layers, 1, cfg->se_act, cfg->se_prelu, 0 };
    const float g32 = (float)cfg->gamma;
    const int64_t P = agent_num_params(cfg);
    const int64_t ps = orc_mlp_num_params(&sn), pr = orc_mlp_num_params(&rn);
    /* se_layer_norm: the SE nets evaluated with their (never perturbed) LayerNorm, theta keeps the Linear-only layout */
    orc_mlp_desc sn_e = sn, rn_e = rn, dn_e = dn;
    const float *se_p[3] = { se_params, se_params + ps, se_params + ps + pr };
    float *se_own[3] = { NULL, NULL, NULL };
    if (cfg->se_layer_norm && cfg->se_layers >= 2 && !(cfg->synthetic_env_type == 1)) {
        sn_e.use_layer_norm = rn_e.use_layer_norm = dn_e.use_layer_norm = 1;
        se_own[0] = mlp_with_unit_layer_norm(&sn, se_p[0]); se_own[1] = mlp_with_unit_layer_norm(&rn, se_p[1]); se_own[2] = mlp_with_unit_layer_norm(&dn, se_p[2]);
        for (int i = 0; i < 3; ++i) se_p[i] = se_own[i];
    }
    if (cfg->se_layer_norm && cfg->se_layers >= 2 && reward_env && rtype != 0) {      /* the reward net's own LayerNorm, likewise */
        se_own[0] = mlp_with_unit_layer_norm(&rd, se_params);
        rd.use_layer_norm = 1; se_params = se_own[0];
    }
    const int64_t row_stride = 2 * S + 3;
    int64_t cap = (int64_t)cfg->train_episodes * cfg->max_steps;
    if (cap > cfg->rb_size) cap = cfg->rb_size;
    if (cap < 1) cap = 1;

    float *online = malloc(sizeof(float) * P), *target = malloc(sizeof(float) * P);
    float *am = calloc(P, sizeof(float)), *av = calloc(P, sizeof(float));
    float *rb = malloc(sizeof(float) * cap * row_stride);
    float *batch = malloc(sizeof(float) * (int64_t)B * row_stride);
    float (*z)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*a)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    double *test_returns = malloc(sizeof(double) * (cfg->test_episodes > 0 ? cfg->test_episodes : 1));
    double *meter = malloc(sizeof(double) * (cfg->train_episodes > 0 ? cfg->train_episodes : 1));
    memcpy(online, agent_init, sizeof(float) * P);
    memcpy(target, agent_init, sizeof(float) * P);  /* model_target.load_state_dict(model.state_dict()) DDQN.py:35 */

    rng_state rng = { cfg, rng_key, tapes, 0, 0, 0, 0, 0 };
    int64_t rb_ptr = 0, rb_size = 0, learn_it = 0, train_steps = 0, test_steps = 0;
    double b1pow = 1.0, b2pow = 1.0;
    double eps = cfg->eps_init;
    int n_meter = 0, episodes_run = 0;
    if (trace) trace->n = 0;

    const int budgeted = cfg->step_budget > 0;
    int timed_out_at = -1;
    for (int episode = 0; episode < cfg->train_episodes; ++episode) {
        /* time_is_up (base_agent.py:90-97): elapsed = env steps taken so far (train + test) */
        if (budgeted && train_steps + test_steps > cfg->step_budget) { timed_out_at = episode; break; }
        /* DDQN.update_parameters_per_episode (DDQN.py:112-117) */
        if (episode == 0) eps = cfg->eps_init;
        else { eps *= cfg->eps_decay; if (eps < cfg->eps_min) eps = cfg->eps_min; }

        double st0[4];
        float state[64], next_state[64], x[64];
        draw_reset(&rng, 1, rng.n_train_ep++, st0);
        real_env_obs(cfg->env_id, st0, state);   /* VirtualEnv.reset / RewardEnv.reset -> fp32 real-env reset state (virtual_env.py:35-41) */
        float phi_cache = 0.0f;                  /* RewardEnv: phi(s) of the state the env is in */
        int have_phi = 0;
        int ep_len = 0, env_steps = 0;
        float ep_reward = 0.0f;                  /* base_agent.py:102,121 episode_reward += reward (fp32 tensors) */
        const int k_rep = cfg->same_action_num > 1 ? cfg->same_action_num : 1;
        for (int t = 0; t < cfg->max_steps; t += k_rep) {                       /* base_agent.py:104 range(0, max_steps, same_action_num) */
            /* select_train_action (DDQN.py:97-104) */
            int act, explored = 0;
            double u = draw_eps_uniform(&rng);
            if (u < eps) { act = draw_rand_action(&rng); explored = 1; }
            else act = agent_greedy_action(cfg, online, state, z, a);
            /* EnvWrapper.step: same_action_num env steps with the one action */
            float reward = 0.0f, done = 0.0f, cur[64];
            memcpy(cur, state, sizeof(float) * S);
            if (reward_env) {
                /* real branch (env_wrapper.py:56-61) over RewardEnv.step (reward_env.py:61-66): the real env's transition (TimeLimit:
                 * done at max_steps), the reward through _calc_reward with the perturbed reward network (se_params); the repeats stop
                 * at done, the shaped rewards are summed as python floats */
                double rsum = 0.0;
                int dn_i = 0;
                for (int r_ = 0; r_ < k_rep; ++r_) {
                    double rew;
                    real_env_step(cfg->env_id, st0, act, &rew, &dn_i);
                    ++env_steps;
                    if (env_steps >= cfg->max_steps) dn_i = 1;
                    real_env_obs(cfg->env_id, st0, next_state);
                    const float sh = rn_shape_one(rtype, S, 0, &rd, se_params, g32, cur, next_state, NULL, (float)rew, &phi_cache, have_phi, z, a);
                    have_phi = 1;
                    rsum = rsum + (double)sh;
                    memcpy(cur, next_state, sizeof(float) * S);
                    if (dn_i) break;
                }
                reward = (float)rsum;
                done = dn_i ? 1.0f : 0.0f;
            } else {
                /* virtual branch (env_wrapper.py:17-29) over VirtualEnv.step: every repeat runs whatever the done flag says, the fp32
                 * rewards are added up, the last state / done flag are returned */
                for (int r_ = 0; r_ < k_rep; ++r_) {
                    float r1;
                    for (int i = 0; i < A; ++i) x[i] = (i == act) ? 1.0f : 0.0f;
                    for (int i = 0; i < S; ++i) x[A + i] = cur[i];
                    mlp_forward_one(&sn_e, se_p[0], x, next_state, z, a);
                    mlp_forward_one(&rn_e, se_p[1], x, &r1, z, a);
                    mlp_forward_one(&dn_e, se_p[2], x, &done, z, a);
                    reward = r_ == 0 ? r1 : reward + r1;
                    memcpy(cur, next_state, sizeof(float) * S);
                }
            }
            /* ReplayBuffer.add (utils.py:24-32) */
            float *row = rb + rb_ptr * row_stride;
            memcpy(row, state, sizeof(float) * S);
            row[S] = (float)act;
            memcpy(row + S + 1, next_state, sizeof(float) * S);
            row[2 * S + 1] = reward; row[2 * S + 2] = done;
            rb_ptr = (rb_ptr + 1) % cap;
            if (rb_size < cap) ++rb_size;
            float loss = NAN;
            if (episode >= cfg->init_episodes) {
                for (int b = 0; b < B; ++b) {
                    int idx = draw_replay_idx(&rng, learn_it, b, rb_size);
                    if (idx < 0 || idx >= rb_size) { rng.err = -6; idx = 0; }
                    memcpy(batch + (int64_t)b * row_stride, rb + (int64_t)idx * row_stride, sizeof(float) * row_stride);
                }
                ++learn_it;
                if (cfg->icm_enabled) {          /* DDQN.py:74-76 / DuelingDDQN.py: icm.train, then rewards += intrinsic rewards */
                    icm_train_and_reward(&icm, &ihp, icm_p, icm_m, icm_v, icm_pows, batch, row_stride, S + 1, 1, B, r_intr);
                    for (int b = 0; b < B; ++b) batch[(int64_t)b * row_stride + 2 * S + 1] = batch[(int64_t)b * row_stride + 2 * S + 1] + r_intr[b];
                }
                loss = cfg->agent_kind == 1 ? orc_dueling_learn(cfg, online, target, am, av, &b1pow, &b2pow, batch, row_stride)
                                            : orc_ddqn_learn(cfg, online, target, am, av, learn_it, &b1pow, &b2pow, batch, row_stride);
            }
            if (trace && trace->n < trace->cap) {
                int64_t k = trace->n++;
                trace->episode[k] = episode; trace->action[k] = act; trace->explored[k] = explored;
                memcpy(trace->state + k * S, state, sizeof(float) * S);
                memcpy(trace->next_state + k * S, next_state, sizeof(float) * S);
                trace->reward[k] = reward; trace->done[k] = done; trace->loss[k] = loss;
            }
            memcpy(state, next_state, sizeof(float) * S);
            ep_reward = ep_reward + reward;
            ep_len += k_rep; ++train_steps;                                         /* base_agent.py:122 episode_length += same_action_num */
            if (done > 0.5f) break;
        }
        ++episodes_run;
        if (episode_len) episode_len[episode] = ep_len;
        double tm;
        if (cfg->test_mode == 1) tm = (double)ep_reward;      /* train(env, test_env=None): avg_meter_reward.update(episode_reward) (base_agent.py:138) */
        else {
            /* per-episode test on the real env (base_agent.py:134-136) */
            run_test_phase(cfg, &qd, online, &rng, test_returns, &test_steps, z, a);
            tm = mean_seq(test_returns, cfg->test_episodes);
        }
        meter[n_meter++] = tm;
        if (episode_test_mean) episode_test_mean[episode] = tm;
        /* early out (base_agent.py:49-62,141-148): break_env = the test env (real rule), or without one the training env itself */
        if (episode >= cfg->init_episodes &&
            meter_env_solved(meter, n_meter, cfg->early_out_num, cfg->test_mode == 1 && !reward_env, cfg->solved_reward, cfg->early_out_virtual_diff,
                             episode, cfg->init_episodes)) break;
    }
    if (timed_out_at >= 0) budget_pad_train(episode_test_mean, episode_len, meter, n_meter, episodes_run, cfg->train_episodes);
    else for (int e = episodes_run; e < cfg->train_episodes; ++e) {
        if (episode_test_mean) episode_test_mean[e] = NAN;
        if (episode_len) episode_len[e] = 0;
    }
    /* final test (GTN_worker.py:199) with the time that is left (GTN_worker.py:199 time_remaining - elapsed) */
    if (budgeted) run_test_phase_budget(cfg, &qd, online, &rng, test_returns, &test_steps, z, a, cfg->step_budget - (train_steps + test_steps));
    else run_test_phase(cfg, &qd, online, &rng, test_returns, &test_steps, z, a);
    if (final_test_returns) memcpy(final_test_returns, test_returns, sizeof(double) * cfg->test_episodes);
    if (res) {
        res->score = mean_seq(test_returns, cfg->test_episodes);
        res->episodes_run = episodes_run; res->train_steps = train_steps;
        res->learn_steps = learn_it; res->test_steps = test_steps;
    }
    if (cfg->icm_enabled && icm_final) memcpy(icm_final, icm_p, sizeof(float) * icm.P);
    if (final_online) memcpy(final_online, online, sizeof(float) * P);
    free(icm_p); free(icm_m); free(icm_v); free(r_intr);
    free(online); free(target); free(am); free(av); free(rb); free(batch); free(z); free(a); free(test_returns); free(meter);
    free(se_own[0]); free(se_own[1]); free(se_own[2]);
    return rng.err;
}

/* ------------------------------------------------------------------------------------------
 * population driver: worker p runs chains {3p: theta, 3p+1: theta+eps_p, 3p+2: theta-eps_p}
 * (GTN_worker.py:84-102), threads over chains.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const orc_ddqn_cfg *cfg; const float *theta, *eps, *agent_init;
    int64_t pop, p_theta, p_agent, worker_offset; uint64_t seed, generation;
    double *scores; orc_chain_result *results;
    int64_t next; pthread_mutex_t mu; int err;
} pop_job;

static void *pop_thread(void *arg)
{
    pop_job *j = (pop_job *)arg;
    float *w = malloc(sizeof(float) * j->p_theta);
    for (;;) {
        pthread_mutex_lock(&j->mu);
        int64_t c = j->next++;
        pthread_mutex_unlock(&j->mu);
        if (c >= 3 * j->pop) break;
        int64_t p = c / 3; int kind = (int)(c % 3);
        float sign = kind == 0 ? 0.0f : (kind == 1 ? 1.0f : -1.0f);
        const float *e = j->eps + p * j->p_theta;
        for (int64_t i = 0; i < j->p_theta; ++i) w[i] = fmaf(sign, e[i], j->theta[i]);
        orc_chain_result r;
        int rc = orc_ddqn_se_chain(j->cfg, w, j->agent_init + c * j->p_agent,
                                   orc_chain_key(j->seed, j->generation, (uint64_t)(j->worker_offset + p), (uint64_t)kind),
                                   NULL, NULL, NULL, NULL, NULL, &r);
        if (rc) j->err = rc;
        j->scores[c] = r.score;
        if (j->results) j->results[c] = r;
    }
    free(w);
    return NULL;
}

int orc_ddqn_se_population(const orc_ddqn_cfg *cfg, const float *theta, const float *eps, int64_t pop, int64_t p_theta,
                           const float *agent_init, uint64_t seed, uint64_t generation, int64_t worker_offset,
                           int threads, double *chain_scores, orc_chain_result *results)
{
    pop_job j = { cfg, theta, eps, agent_init, pop, p_theta, agent_num_params(cfg), worker_offset, seed, generation,
                  chain_scores, results, 0, PTHREAD_MUTEX_INITIALIZER, 0 };
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    pthread_t th[256];
    for (int t = 0; t < threads; ++t) pthread_create(&th[t], NULL, pop_thread, &j);
    for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
    return j.err;
}

/* ------------------------------------------------------------------------------------------
 * config 4: QL on a RewardEnv over a grid MDP
 * ---------------------------------------------------------------------------------------- */
/* phi(s) = reward_net(one_hot(s)) (reward_env.py:74-76) and the shaped reward of every (s,a):
 * type 0: r; 1: g*phi(s') - phi(s); 2: r + g*phi(s') - phi(s); 5: phi(s'); 6: r + phi(s')  (reward_env.py:81-110),
 * evaluated left to right in fp32 exactly like the torch expression, result `.item()`. */
int orc_rn_shaped_rewards(const orc_ql_cfg *cfg, const float *rn_params, const int32_t *next_state, const double *reward,
                          float *phi_out, float *shaped)
{
    const int N = cfg->n_states, A = cfg->n_actions;
    if (N > ORC_MAX_WIDTH || cfg->rn_hidden > ORC_MAX_WIDTH || cfg->rn_layers > ORC_MAX_LAYERS || cfg->rn_layers < 1) return -1;
    const int t = cfg->reward_env_type;
    if (!(t == 0 || t == 1 || t == 2 || t == 5 || t == 6)) return -1;
    orc_mlp_desc rd = { N, cfg->rn_hidden, cfg->rn_layers, 1, cfg->rn_act, cfg->rn_prelu, 0 };
    float *rn_own = NULL;               /* the ENV section's use_layer_norm: see mlp_with_unit_layer_norm */
    if (cfg->rn_layer_norm && cfg->rn_layers >= 2 && t != 0) { rn_own = mlp_with_unit_layer_norm(&rd, rn_params); rd.use_layer_norm = 1; rn_params = rn_own; }
    float *phi = malloc(sizeof(float) * N);
    float *x = calloc(N, sizeof(float));
    float (*z)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    float (*a)[ORC_MAX_WIDTH] = malloc(sizeof(float) * ORC_MAX_LAYERS * ORC_MAX_WIDTH);
    for (int s = 0; s < N; ++s) {
        if (t == 0) { phi[s] = 0.0f; continue; }     /* type 0 builds a dummy 1-input net that is never evaluated */
        x[s] = 1.0f;
        mlp_forward_one(&rd, rn_params, x, &phi[s], z, a);
        x[s] = 0.0f;
    }
    const float g32 = (float)cfg->gamma;
    for (int s = 0; s < N; ++s)
        for (int ac = 0; ac < A; ++ac) {
            const int s2 = next_state[s * A + ac];
            const float r32 = (float)reward[s * A + ac];
            float v;
            switch (t) {
            case 0: v = r32; break;
            case 1: v = g32 * phi[s2] - phi[s]; break;
            case 2: v = (r32 + g32 * phi[s2]) - phi[s]; break;
            case 5: v = phi[s2]; break;
            default: v = r32 + phi[s2]; break;
            }
            shaped[s * A + ac] = v;
        }
    if (phi_out) memcpy(phi_out, phi, sizeof(float) * N);
    free(phi); free(x); free(z); free(a); free(rn_own);
    return 0;
}

static int ql_argmax_f32(const double *row, int n)
{
    /* torch.argmax(torch.tensor(row)) (QL.py:93-94,98-99): the fp64 row is cast to fp32 first; first maximum wins */
    int best = 0;
    float bv = (float)row[0];
    for (int i = 1; i < n; ++i) { float v = (float)row[i]; if (v > bv) { bv = v; best = i; } }
    return best;
}

int orc_ql_rn_chain(const orc_ql_cfg *cfg, const float *rn_params, const float *shaped_override, const int32_t *next_state,
                    const double *reward, const uint8_t *done_tab, uint64_t rng_key, const orc_tapes *tapes, double *episode_test_mean,
                    int32_t *episode_len, double *final_test_returns, double *q_table_out, orc_ql_trace *trace,
                    orc_chain_result *res)
{
    const int N = cfg->n_states, A = cfg->n_actions;
    if (cfg->rng_mode == ORC_RNG_TAPE && !tapes) return -1;
    float *shaped = malloc(sizeof(float) * N * A);
    if (shaped_override) memcpy(shaped, shaped_override, sizeof(float) * N * A);   /* parity tests: the reference's own table */
    else if (orc_rn_shaped_rewards(cfg, rn_params, next_state, reward, NULL, shaped)) { free(shaped); return -1; }
    double *q = calloc((size_t)N * A, sizeof(double));       /* q_table = [[0]*A for _ in range(N)]  QL.py:25 */
    int64_t *visits = calloc((size_t)N * A, sizeof(int64_t)); /* visitation_table n(s,a)  QL.py:31 */
    double *meter = malloc(sizeof(double) * (cfg->train_episodes > 0 ? cfg->train_episodes : 1));
    double *rets = malloc(sizeof(double) * (cfg->test_episodes > 0 ? cfg->test_episodes : 1));
    int64_t *tlens = malloc(sizeof(int64_t) * (cfg->test_episodes > 0 ? cfg->test_episodes : 1));
    int64_t n_eps = 0, n_act = 0, train_steps = 0, learn_steps = 0, test_steps = 0;
    int err = 0, episodes_run = 0, n_meter = 0, timed_out = 0;
    double eps = cfg->eps_init;
    const int k_rep = cfg->same_action_num > 1 ? cfg->same_action_num : 1;
    if (trace) trace->n = 0;

#define QL_TEST_PHASE()                                                                                       \
    for (int te = 0; te < cfg->test_episodes; ++te) {                                                         \
        int s = cfg->start_state;                                                                             \
        float ep_reward = 0.0f;                                                                               \
        tlens[te] = 0;                                                                                        \
        int dn = 0;                                                                                           \
        for (int t = 0; t < cfg->max_steps && !dn; t += k_rep) {                                              \
            int ac = ql_argmax_f32(q + (size_t)s * A, A);                                                     \
            double rsum_ = 0.0;                               /* EnvWrapper.step: python-float sum, stop at done */ \
            for (int r_ = 0; r_ < k_rep; ++r_) {                                                              \
                dn = done_tab[s * A + ac];                                                                    \
                rsum_ = rsum_ + reward[s * A + ac];                                                           \
                s = next_state[s * A + ac];                                                                   \
                ++test_steps; ++tlens[te];                                                                    \
                if (tlens[te] >= cfg->max_steps) dn = 1;                                                      \
                if (dn) break;                                                                                \
            }                                                                                                 \
            ep_reward = ep_reward + (float)rsum_;                                                             \
        }                                                                                                     \
        rets[te] = (double)ep_reward;                                                                         \
    }

    for (int episode = 0; episode < cfg->train_episodes; ++episode) {
        if (cfg->step_budget > 0 && train_steps + test_steps > cfg->step_budget) { timed_out = 1; break; }   /* time_is_up */
        if (episode == 0) eps = cfg->eps_init;                                  /* QL.py:101-106 */
        else { eps *= cfg->eps_decay; if (eps < cfg->eps_min) eps = cfg->eps_min; }
        int s = cfg->start_state, ep_len = 0, env_steps = 0;                    /* RewardEnv.reset -> real_env.reset() */
        float ep_reward = 0.0f;                                                 /* base_agent.py:121 episode_reward += reward (fp32 tensor) */
        for (int t = 0; t < cfg->max_steps; t += k_rep) {                       /* base_agent.py:104 range(0, max_steps, same_action_num) */
            double u;
            if (cfg->rng_mode == ORC_RNG_TAPE) { if (n_eps >= tapes->n_eps_uniform) { err = -2; u = 1.0; } else u = tapes->eps_uniform[n_eps]; }
            else u = u64_to_unit(orc_rng_u64(rng_key, STREAM_EPS, (uint64_t)n_eps));
            ++n_eps;
            int ac, explored = 0;
            if (u < eps) {
                explored = 1;
                if (cfg->rng_mode == ORC_RNG_TAPE) { if (n_act >= tapes->n_rand_action) { err = -3; ac = 0; } else ac = tapes->rand_action[n_act]; }
                else ac = (int)u64_to_below(orc_rng_u64(rng_key, STREAM_ACTION, (uint64_t)n_act), (uint32_t)A);
                ++n_act;
            } else ac = ql_argmax_f32(q + (size_t)s * A, A);
            /* EnvWrapper.step (env_wrapper.py:56-61) over RewardEnv.step (reward_env.py:61-66) + TimeLimit: the action same_action_num
             * times or until done, the shaped rewards (python floats from .item()) summed and stored as one fp32 value */
            int s2 = s, dn = 0;
            double rsum = 0.0;
            for (int r_ = 0; r_ < k_rep; ++r_) {
                const int sc = s2;
                dn = done_tab[sc * A + ac];
                ++env_steps;
                if (env_steps >= cfg->max_steps) dn = 1;
                rsum = rsum + (double)shaped[sc * A + ac];
                s2 = next_state[sc * A + ac];
                if (dn) break;
            }
            const double r = (double)(float)rsum;
            /* QL.learn (QL.py:37-75) / SARSA.learn (SARSA.py:36-60): batch_size draws of the single stored transition,
             * only once episode >= init_episodes (base_agent.py:127-128) */
            if (episode >= cfg->init_episodes) {
                for (int k = 0; k < cfg->batch_size; ++k) {
                    double boot;
                    if (cfg->agent_kind == 1) {                                     /* next_action = select_train_action(next_state) */
                        double u2;
                        if (cfg->rng_mode == ORC_RNG_TAPE) { if (n_eps >= tapes->n_eps_uniform) { err = -2; u2 = 1.0; } else u2 = tapes->eps_uniform[n_eps]; }
                        else u2 = u64_to_unit(orc_rng_u64(rng_key, STREAM_EPS, (uint64_t)n_eps));
                        ++n_eps;
                        int a2;
                        if (u2 < eps) {
                            if (cfg->rng_mode == ORC_RNG_TAPE) { if (n_act >= tapes->n_rand_action) { err = -3; a2 = 0; } else a2 = tapes->rand_action[n_act]; }
                            else a2 = (int)u64_to_below(orc_rng_u64(rng_key, STREAM_ACTION, (uint64_t)n_act), (uint32_t)A);
                            ++n_act;
                        } else a2 = ql_argmax_f32(q + (size_t)s2 * A, A);
                        boot = q[(size_t)s2 * A + a2];
                    } else {
                        boot = q[(size_t)s2 * A];
                        for (int i = 1; i < A; ++i) if (q[(size_t)s2 * A + i] > boot) boot = q[(size_t)s2 * A + i];
                    }
                    double rr = r;
                    if (cfg->count_based) {                                         /* QL.py:52-55 */
                        visits[(size_t)s * A + ac] += 1;
                        rr += cfg->beta / (sqrt((double)visits[(size_t)s * A + ac]) + 1e-9);
                    }
                    const double delta = rr + cfg->gamma * boot * (dn ? 0.0 : 1.0) - q[(size_t)s * A + ac];
                    q[(size_t)s * A + ac] += cfg->alpha * delta;
                }
                ++learn_steps;
            }
            if (trace && trace->n < trace->cap) {
                int64_t k = trace->n++;
                trace->action[k] = ac | (explored << 16); trace->state[k] = s; trace->next_state[k] = s2;
                trace->reward[k] = (float)r; trace->done[k] = dn ? 1.0f : 0.0f;
            }
            s = s2;
            ep_reward = ep_reward + (float)r;
            ep_len += k_rep; ++train_steps;
            if (dn) break;
        }
        ++episodes_run;
        if (episode_len) episode_len[episode] = ep_len;
        double tm;
        if (cfg->test_mode == 1) tm = (double)ep_reward;      /* train(env, test_env=None): the RewardEnv's own episode reward (base_agent.py:138) */
        else {
            QL_TEST_PHASE()
            tm = mean_seq(rets, cfg->test_episodes);
        }
        meter[n_meter++] = tm;
        if (episode_test_mean) episode_test_mean[episode] = tm;
        if (episode >= cfg->init_episodes &&
            meter_env_solved(meter, n_meter, cfg->early_out_num, 0, cfg->solved_reward, 0.0, episode, cfg->init_episodes)) break;
    }
    if (timed_out) budget_pad_train(episode_test_mean, episode_len, meter, n_meter, episodes_run, cfg->train_episodes);
    else for (int e = episodes_run; e < cfg->train_episodes; ++e) {
        if (episode_test_mean) episode_test_mean[e] = NAN;
        if (episode_len) episode_len[e] = 0;
    }
    {
        const int64_t remaining = cfg->step_budget - (train_steps + test_steps), before = test_steps;
        QL_TEST_PHASE()
        if (cfg->step_budget > 0) test_steps = before + budget_cut_test(rets, tlens, cfg->test_episodes, remaining);
    }
#undef QL_TEST_PHASE
    if (final_test_returns) memcpy(final_test_returns, rets, sizeof(double) * cfg->test_episodes);
    if (q_table_out) memcpy(q_table_out, q, sizeof(double) * N * A);
    if (res) {
        res->score = mean_seq(rets, cfg->test_episodes);
        res->episodes_run = episodes_run; res->train_steps = train_steps; res->learn_steps = learn_steps; res->test_steps = test_steps;
    }
    free(shaped); free(q); free(visits); free(meter); free(rets); free(tlens);
    return err;
}

#include "lenv_oracle_td3.inc"
#include "lenv_oracle_td3d.inc"

/* ------------------------------------------------------------------------------------------
 * NES worker / master math
 * ---------------------------------------------------------------------------------------- */
/* GTN_worker.py:234-254 (num_grad_evals == 1, so 'mean' and 'minmax' coincide) */
void orc_worker_best(const double *score_add, const double *score_sub, int64_t pop, int mirrored, double *score_best, float *sign)
{
    for (int64_t p = 0; p < pop; ++p) {
        if (mirrored) {
            score_best[p] = score_add[p] > score_sub[p] ? score_add[p] : score_sub[p];
            sign[p] = score_sub[p] > score_add[p] ? -1.0f : 1.0f;   /* invert_eps() iff sub > add; ties keep +eps */
        } else {
            score_best[p] = score_add[p];
            sign[p] = 1.0f;
        }
    }
}

/* statistics.mean of python floats is the correctly rounded exact mean; this double-double accumulation (TwoSum per term,
 * one renormalisation, one correction step of the division) reproduces it for the handful of scores a worker averages. */
static double exact_mean(const double *x, int n)
{
    double hi = 0.0, lo = 0.0;
    for (int i = 0; i < n; ++i) {
        const double s = hi + x[i], bb = s - hi, err = (hi - (s - bb)) + (x[i] - bb);
        hi = s; lo = lo + err;
    }
    const double s = hi + lo, e = lo - (s - hi);
    const double q = s / (double)n, r = fma(-q, (double)n, s) + e;
    return q + r / (double)n;
}

/* One generation's stochastic inputs from the counter RNG -- the CPU twin of lenv_nes_draw (csrc/nes_update.hip): eps [pop,P]
 * = (float)N(0,1) * noise_std (GTN_Worker.get_random_noise, GTN_worker.py:156-163), agent_init [chains,p_agent] =
 * (2u-1)*bound (nn.Linear default init of a fresh agent), rng_keys [chains].  Any output may be NULL. */
void orc_nes_draw(uint64_t seed, uint64_t generation, int64_t pop, int64_t P, float noise_std, float *eps, int64_t chains,
                  int64_t cpw, int64_t worker_lo, int64_t p_agent, const float *bounds, float *agent_init, uint64_t *rng_keys)
{
    const uint64_t eps_domain = 0x6e65735f657073ULL;
    if (eps)
        for (int64_t w = 0; w < pop; ++w) {
            const uint64_t key = orc_chain_key(seed ^ eps_domain, generation, (uint64_t)w, 0);
            for (int64_t i = 0; i < P; ++i) eps[w * P + i] = (float)orc_normal(key, 9, (uint64_t)i) * noise_std;
        }
    for (int64_t c = 0; c < chains; ++c) {
        const uint64_t key = orc_chain_key(seed, generation, (uint64_t)(worker_lo + c / cpw), (uint64_t)(c % cpw));
        if (rng_keys) rng_keys[c] = key;
        if (agent_init)
            for (int64_t i = 0; i < p_agent; ++i) {
                const float u = (float)u64_to_unit(orc_rng_u64(key, 10, (uint64_t)i));
                agent_init[c * p_agent + i] = (u * 2.0f - 1.0f) * bounds[i];
            }
    }
}

/* GTN_worker.py:234-254 with num_grad_evals = G score lists per direction: grad_eval_type 0 = 'mean' (statistics.mean),
 * 1 = 'minmax' (min of BOTH lists, as the reference does) */
int orc_worker_best_multi(const double *score_add /*[pop,G]*/, const double *score_sub /*[pop,G]*/, int64_t pop, int G, int mirrored,
                          int grad_eval_type, double *score_best, float *sign)
{
    if (G < 1 || (grad_eval_type != 0 && grad_eval_type != 1)) return -1;
    for (int64_t p = 0; p < pop; ++p) {
        double a, b;
        if (grad_eval_type == 0) { a = exact_mean(score_add + p * G, G); b = exact_mean(score_sub + p * G, G); }
        else {
            a = score_add[p * G]; b = score_sub[p * G];
            for (int i = 1; i < G; ++i) { if (score_add[p * G + i] < a) a = score_add[p * G + i]; if (score_sub[p * G + i] < b) b = score_sub[p * G + i]; }
        }
        if (mirrored) { score_best[p] = a > b ? a : b; sign[p] = b > a ? -1.0f : 1.0f; }
        else { score_best[p] = a; sign[p] = 1.0f; }
    }
    return 0;
}

/* rank helpers with a documented stable order (np.argsort's tie order is implementation-defined,
 * SURVEY.md Appendix A #14): among equal scores the lower index comes first. */
static void argsort_stable(const double *v, int64_t n, int descending, int64_t *idx)
{
    for (int64_t i = 0; i < n; ++i) idx[i] = i;
    for (int64_t i = 1; i < n; ++i) {           /* insertion sort: stable */
        int64_t k = idx[i], j = i - 1;
        while (j >= 0 && (descending ? v[idx[j]] < v[k] : v[idx[j]] > v[k])) { idx[j + 1] = idx[j]; --j; }
        idx[j + 1] = k;
    }
}

/* np.add.reduce of a contiguous double array = numpy's pairwise summation: fewer than 8 elements are added left to right;
 * up to 128 go through eight interleaved accumulators r[j] += a[8k + j], combined as ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)),
 * the n % 8 leftover elements added to that one by one; above 128 the array is split at n/2 rounded down to a multiple of 8 and
 * the two halves' sums are added.  (The reduction starts from the identity 0.0, which changes no finite sum.) */
static double numpy_pairwise_sum(const double *a, int64_t n)
{
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        int64_t i;
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_pairwise_sum(a, n2) + numpy_pairwise_sum(a + n2, n - n2);
}

double orc_numpy_sum(const double *a, int64_t n) { return numpy_pairwise_sum(a, n); }

int orc_score_transform(int type, const double *scores_in, const double *scores_orig, int64_t n, double *out)
{
    double *scores = malloc(sizeof(double) * n);
    int64_t *s = malloc(sizeof(int64_t) * n);
    memcpy(scores, scores_in, sizeof(double) * n);
    int rc = 0;
    if (type == 0) {
        double mn = scores[0], mx = scores[0];
        for (int64_t i = 1; i < n; ++i) { if (scores[i] < mn) mn = scores[i]; if (scores[i] > mx) mx = scores[i]; }
        for (int64_t i = 0; i < n; ++i) scores[i] = (scores[i] - mn) / (mx - mn + 1e-9);
    } else if (type == 1) {
        argsort_stable(scores_in, n, 0, s);
        for (int64_t i = 0; i < n; ++i) scores[s[i]] = (double)i / (double)(n - 1);
    } else if (type == 2 || type == 3) {
        argsort_stable(scores_in, n, 1, s);       /* np.argsort(-scores) */
        for (int64_t i = 0; i < n; ++i) scores[s[i]] = (double)(i + 1);
        double lg = log((double)n / 2 + 1), sum = 0.0;
        for (int64_t i = 0; i < n; ++i) { double u = lg - log(scores[i]); scores[i] = u > 0 ? u : 0; }
        for (int64_t i = 0; i < n; ++i) sum += scores[i];   /* python sum(): sequential */
        for (int64_t i = 0; i < n; ++i) scores[i] = scores[i] / sum;
        if (type == 2) for (int64_t i = 0; i < n; ++i) scores[i] -= 1.0 / (double)n;
        double mx = scores[0];
        for (int64_t i = 1; i < n; ++i) if (scores[i] > mx) mx = scores[i];
        for (int64_t i = 0; i < n; ++i) scores[i] /= mx;
    } else if (type == 4) {
        int64_t am = 0;
        for (int64_t i = 1; i < n; ++i) if (scores_in[i] > scores_in[am]) am = i;
        for (int64_t i = 0; i < n; ++i) scores[i] = i == am ? 1.0 : 0.0;
    } else if (type == 5 || type == 6 || type == 7) {
        const double avg = numpy_pairwise_sum(scores_orig, n) / (double)n;       /* np.mean(scores_orig) */
        int64_t cnt = 0, am = 0;
        double mx = scores_in[0];
        for (int64_t i = 0; i < n; ++i) { if (scores_in[i] > avg + 1e-6) ++cnt; if (scores_in[i] > mx) { mx = scores_in[i]; am = i; } }
        if (cnt > 0) {
            if (type == 5) {
                for (int64_t i = 0; i < n; ++i) scores[i] = i == am ? 1.0 : 0.0;
            } else {
                for (int64_t i = 0; i < n; ++i) {
                    double idx = scores_in[i] > avg + 1e-6 ? 1.0 : 0.0;
                    scores[i] = idx * (scores_in[i] - avg) / (mx - avg + 1e-9);
                }
                if (type == 6) {
                    double m2 = scores[0];
                    for (int64_t i = 1; i < n; ++i) if (scores[i] > m2) m2 = scores[i];
                    for (int64_t i = 0; i < n; ++i) scores[i] /= m2;
                } else {
                    double s2 = 0.0;
                    for (int64_t i = 0; i < n; ++i) s2 += scores[i];
                    for (int64_t i = 0; i < n; ++i) scores[i] /= s2;
                }
            }
        } else {
            for (int64_t i = 0; i < n; ++i) scores[i] = 0.0;
        }
    } else {
        rc = -1;   /* ValueError("Unknown rank transform type") GTN_master.py:263 */
    }
    if (!rc) memcpy(out, scores, sizeof(double) * n);
    free(scores); free(s);
    return rc;
}

/* GTN_master.py:267-298 */
void orc_update_env(float *theta, const float *eps, const float *sign, const double *weights, int64_t pop, int64_t p_theta,
                    const uint8_t *linear_mask, double step_size, int nes_step_size, double weight_decay)
{
    double ss = step_size;
    if (nes_step_size) ss = ss / (double)pop;
    const float decay = (float)(1.0 - weight_decay);
    for (int64_t i = 0; i < p_theta; ++i)
        if (!linear_mask || linear_mask[i]) theta[i] = theta[i] * decay;
    for (int64_t w = 0; w < pop; ++w) {
        const float c = (float)(ss * weights[w]);        /* python: (ss * score_transform) * tensor */
        const float *e = eps + w * p_theta;
        for (int64_t i = 0; i < p_theta; ++i)
            if (!linear_mask || linear_mask[i]) theta[i] = theta[i] + c * (sign[w] * e[i]);
    }
}
