"""The one-step API kernels (mlp_forward.hip, se_step.hip, qnet_td.hip, rn_shape_rows.hip) at the shapes that cross their
thread strides, tiles and block counts.

Every case is held bit for bit against the CPU oracle and, to catch a slip shared by kernel and oracle, against an fp64 forward
written here as plain numpy matrix products.  Tolerance against the fp64 forward, u = 2^-24:
  * nets without LayerNorm: the running bound computed beside the forward.  Per layer e_z = |W| e_in + (n_in + 1) u (|W| |a| + |b|)
    (n_in fused multiply-adds and the bias addition, each rounding once); a piecewise-linear activation has slope <= 1 and adds
    u |a|; tanh has slope <= 1 and adds 2.4e-7, the bound tests/test_oracle_golden.py holds the oracle's tanh to.
  * LayerNorm nets: the division by a small standard deviation has no useful a-priori bound, so the oracle's largest deviation
    from the fp64 forward on these very inputs was measured on the CPU (LN_MEASURED, beside the parametrizations) and 4x that is
    allowed -- the order of the two statistics' sums is the only freedom an implementation has beyond the oracle's.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ACTS = ["identity", "relu", "leakyrelu", "tanh", "prelu"]
U = 2.0 ** -24
TANH_ERR = 2.4e-7
PRELU = 0.25


@pytest.fixture(scope="module")
def eng():
    from learning_environments_amd import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------
# parameters in the flat layout of lenv_mlp_desc, and the fp64 forward with its error bound
# ---------------------------------------------------------------------------------------------------------------
def make_params(rng, in_dim, hidden, layers, out_dim, layer_norm):
    """W0 b0 | W1 b1 [ln_w ln_b] | W2 b2 ... | Wout bout, every Linear U(-1, 1) / sqrt(fan_in), the LayerNorm's weight in
    [0.5, 1.5] and bias in [-0.2, 0.2] (not the identity it is initialised to)."""
    parts, n_in = [], in_dim
    for l in range(layers):
        parts += [rng.uniform(-1, 1, hidden * n_in) / np.sqrt(n_in), rng.uniform(-1, 1, hidden) / np.sqrt(n_in)]
        if layer_norm and l == 1:
            parts += [rng.uniform(0.5, 1.5, hidden), rng.uniform(-0.2, 0.2, hidden)]
        n_in = hidden
    parts += [rng.uniform(-1, 1, out_dim * n_in) / np.sqrt(n_in), rng.uniform(-1, 1, out_dim) / np.sqrt(n_in)]
    return np.concatenate(parts).astype(np.float32)


def act64(act, z, e):
    a = np.abs
    if act == "identity":
        return z, e
    if act == "relu":
        y = np.maximum(z, 0.0)
    elif act == "leakyrelu":
        y = np.where(z > 0, z, z * float(np.float32(0.01)))
    elif act == "prelu":
        y = np.where(z > 0, z, z * float(np.float32(PRELU)))
    else:
        y = np.tanh(z)
        return y, e + TANH_ERR
    return y, e + U * a(y)


def fwd64(in_dim, hidden, layers, out_dim, act, layer_norm, params, x):
    """(y, e): the net in fp64 and the bound on |fp32 result - y| (e is NaN behind a LayerNorm: no a-priori bound)."""
    p = params.astype(np.float64)
    a, e = x.astype(np.float64), np.zeros(x.shape)
    off, n_in = 0, in_dim
    ln_w = ln_b = None

    def linear(a, e, n_out, n_in, off):
        W = p[off:off + n_out * n_in].reshape(n_out, n_in)
        b = p[off + n_out * n_in:off + n_out * n_in + n_out]
        z = a @ W.T + b
        ez = e @ np.abs(W).T + (n_in + 1) * U * (np.abs(a) @ np.abs(W).T + np.abs(b))
        return z, ez, off + n_out * n_in + n_out

    for l in range(layers):
        z, e, off = linear(a, e, hidden, n_in, off)
        if layer_norm and l >= 1:
            if l == 1:
                ln_w, ln_b = p[off:off + hidden], p[off + hidden:off + 2 * hidden]
                off += 2 * hidden
            mean = z.mean(axis=1, keepdims=True)
            var = ((z - mean) ** 2).mean(axis=1, keepdims=True)
            z = (z - mean) / np.sqrt(var + float(np.float32(1e-5))) * ln_w + ln_b
            e = np.full(z.shape, np.nan)
        a, e = act64(act, z, e)
        n_in = hidden
    y, e, off = linear(a, e, out_dim, n_in, off)
    assert off == p.size
    return y, e


def check_against_fp64(got, y, e, ln_allow, msg):
    """Within the running bound where there is one; a LayerNorm net within 4x the oracle's measured deviation."""
    err = np.abs(got.astype(np.float64) - y)
    if np.isnan(e).any():
        assert err.max() <= 4.0 * ln_allow, (msg, err.max(), ln_allow)
    else:
        assert (err <= e).all(), (msg, (err - e).max())
    return err.max()


# ---------------------------------------------------------------------------------------------------------------
# lenv_mlp_forward: the 256-thread stride over hidden and output units, one workgroup per row
# ---------------------------------------------------------------------------------------------------------------
# largest |oracle - fp64 forward| over the LayerNorm configurations of one (hidden, activation) case, measured on the CPU
# (hidden 1: the variance of one value is 0, every normalised value is the LayerNorm's bias and the deviation is rounding of the rest)
LN_MEASURED_MLP = {
    (1, "identity"): 6.14e-08, (1, "relu"): 6.58e-08, (1, "leakyrelu"): 5.61e-08, (1, "tanh"): 6.57e-08, (1, "prelu"): 5.61e-08,
    (255, "identity"): 2.03e-06, (255, "relu"): 1.02e-06, (255, "leakyrelu"): 1.37e-06, (255, "tanh"): 1.32e-06, (255, "prelu"): 1.40e-06,
    (256, "identity"): 1.98e-06, (256, "relu"): 1.10e-06, (256, "leakyrelu"): 1.45e-06, (256, "tanh"): 1.36e-06, (256, "prelu"): 1.63e-06,
    (257, "identity"): 1.95e-06, (257, "relu"): 1.21e-06, (257, "leakyrelu"): 1.51e-06, (257, "tanh"): 1.05e-06, (257, "prelu"): 1.36e-06,
    (600, "identity"): 2.91e-06, (600, "relu"): 1.71e-06, (600, "leakyrelu"): 2.04e-06, (600, "tanh"): 1.80e-06, (600, "prelu"): 2.19e-06,
}


def mlp_configs(hidden, act):
    for in_dim in (1, 257):
        for out_dim in (1, 300):
            for layers in (1, 2, 3):
                for ln in (False, True):
                    rng = np.random.RandomState(1000 * hidden + 100 * in_dim % 97 + 10 * layers + out_dim % 7 + int(ln) + 31 * ACTS.index(act))
                    params = make_params(rng, in_dim, hidden, layers, out_dim, ln and layers >= 2)
                    x = rng.uniform(-2, 2, (70, in_dim)).astype(np.float32)
                    yield in_dim, out_dim, layers, ln, params, x


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("hidden", [1, 255, 256, 257, 600])
def test_mlp_forward_shapes(eng, orc, hidden, act):
    """in {1, 257} x out {1, 300} x layers 1-3 x LayerNorm on/off, launched with 70, 3 and 1 rows (the rows of the smaller launches
    are the first of the 70, so one oracle and one fp64 forward serve all three)."""
    for in_dim, out_dim, layers, ln, params, x in mlp_configs(hidden, act):
        msg = "in %d hidden %d out %d layers %d %s ln %d" % (in_dim, hidden, out_dim, layers, act, ln)
        d = eng.mlp_desc(in_dim, hidden, layers, out_dim, act, PRELU, ln)
        assert eng.mlp_num_params(d) == params.size, msg
        want = orc.mlp_forward(orc.mlp_desc(in_dim, hidden, layers, out_dim, act, PRELU, ln), params, x)
        y, e = fwd64(in_dim, hidden, layers, out_dim, act, ln, params, x)
        d_params = dev(params)
        for rows in (70, 3, 1):
            got = eng.mlp_forward(d, d_params, dev(x[:rows])).cpu().numpy()
            assert np.array_equal(got, want[:rows]), (msg, rows)
            check_against_fp64(got, y[:rows], e[:rows], LN_MEASURED_MLP.get((hidden, act), 0.0), msg)


def tanh_scan_inputs():
    """Both sides of every 1/16 grid point and of every midpoint between two (where the table entry changes), +-TMAX and its
    neighbours, +-0, denormals, +-inf."""
    k = np.arange(0, 148, dtype=np.float64)
    pts = np.concatenate([k / 16.0, (k + 0.5) / 16.0]).astype(np.float32)
    tmax = np.float32(9.12499905)
    pts = np.concatenate([pts, [tmax, np.float32(9.125), np.float32(1e-45), np.float32(1e-40), np.float32(1.1754942e-38),
                                np.float32(1.17549435e-38), np.float32(0.0), np.float32(np.inf), np.float32(3.4028235e38)]]).astype(np.float32)
    with np.errstate(over="ignore"):                                       # the neighbour above FLT_MAX is inf
        pts = np.concatenate([np.nextafter(pts, np.float32(-np.inf)), pts, np.nextafter(pts, np.float32(np.inf))])
    return np.unique(np.concatenate([pts, -pts]).astype(np.float32))


def test_mlp_forward_tanh_scan(eng, orc):
    """A 1-1-1 tanh net with weights 1 and biases 0, one row per input: y = fma(tanh(fma(x, 1, 0) + 0), 1, 0) + 0 = tanh(x), so the
    device tanh is read at every table-cell edge.  Equal to orc.tanhf in every bit (the net's `+ 0` turns a -0 into +0, so a zero
    is compared as a value), within 2.4e-7 of np.tanh.  NaN inputs are out of scope: no env or agent produces one and neither
    side defines what it returns."""
    x = tanh_scan_inputs()
    assert np.isinf(x).sum() == 2 and (x == 0).any() and (np.abs(x[x != 0]) < 1.2e-38).any() and not np.isnan(x).any()
    params = np.array([1.0, 0.0, 1.0, 0.0], np.float32)
    d = eng.mlp_desc(1, 1, 1, 1, "tanh")
    got = eng.mlp_forward(d, dev(params), dev(x.reshape(-1, 1))).cpu().numpy().reshape(-1)
    want = orc.tanhf(x)
    nz = want != 0
    assert np.array_equal(got[nz].view(np.uint32), want[nz].view(np.uint32))
    assert not got[~nz].any()
    assert np.array_equal(got, orc.mlp_forward(orc.mlp_desc(1, 1, 1, 1, "tanh"), params, x.reshape(-1, 1)).reshape(-1))
    assert np.abs(got.astype(np.float64) - np.tanh(x.astype(np.float64))).max() <= TANH_ERR
    assert got[np.isposinf(x)][0] == 1.0 and got[np.isneginf(x)][0] == -1.0


# ---------------------------------------------------------------------------------------------------------------
# lenv_qnet_td_forward: tiles of 256 samples
# ---------------------------------------------------------------------------------------------------------------
def td_case(S, A, H, batch, chains=3):
    """Three chains with their own online / target nets over a replay of 97 rows; chain 2's online output rows are all the same,
    so every next-state Q-value of that chain ties and the first action must be taken."""
    rng = np.random.RandomState(7000 + 100 * S + 10 * A + H + batch)
    cap, stride = 97, 2 * S + 3 + 2
    online = np.stack([make_params(rng, S, H, 1, A, False) for _ in range(chains)])
    target = np.stack([make_params(rng, S, H, 1, A, False) for _ in range(chains)])
    w2 = S * H + H
    online[2, w2:w2 + A * H] = np.tile(online[2, w2:w2 + H], A)
    online[2, w2 + A * H:] = online[2, w2 + A * H]
    replay = rng.uniform(-1.5, 1.5, (chains, cap, stride)).astype(np.float32)
    replay[:, :, S] = rng.randint(0, A, (chains, cap))
    replay[:, :, 2 * S + 2] = rng.randint(0, 2, (chains, cap))               # done in {0, 1}
    idx = rng.randint(0, cap, (chains, batch)).astype(np.int32)
    idx[:, -1] = cap - 1
    return online, target, replay, idx


@pytest.mark.parametrize("H", [1, 57, 300])
@pytest.mark.parametrize("batch", [1, 255, 256, 257, 600])
def test_qnet_td_forward_tiles(eng, orc, batch, H):
    gamma = 0.99
    for S in (1, 8):
        for A in (1, 4):
            act = ACTS[(S + A + H + batch) % 5]
            msg = "batch %d S %d A %d H %d %s" % (batch, S, A, H, act)
            online, target, replay, idx = td_case(S, A, H, batch)
            qd = eng.mlp_desc(S, H, 1, A, act, PRELU)
            q_sa, y = eng.qnet_td_forward(qd, dev(online), dev(target), dev(replay), dev(idx), gamma)
            q_sa, y = q_sa.cpu().numpy(), y.cpu().numpy()
            od = orc.mlp_desc(S, H, 1, A, act, PRELU)
            for c in range(online.shape[0]):
                rows = replay[c][idx[c]]
                oq, oy, oam = orc.qnet_td_forward(od, online[c], target[c], rows, S, gamma)
                assert np.array_equal(q_sa[c], oq) and np.array_equal(y[c], oy), (msg, c)
                s, a, s2, r, done = rows[:, :S], rows[:, S].astype(np.int64), rows[:, S + 1:2 * S + 1], rows[:, 2 * S + 1], rows[:, 2 * S + 2]
                assert set(np.unique(done)) <= {0.0, 1.0}
                qs, es = fwd64(S, H, 1, A, act, False, online[c], s)
                qn, en = fwd64(S, H, 1, A, act, False, online[c], s2)
                qt, et = fwd64(S, H, 1, A, act, False, target[c], s2)
                b = np.arange(batch)
                assert (np.abs(q_sa[c] - qs[b, a]) <= es[b, a]).all(), (msg, c)
                if c == 2:
                    assert not oam.any(), (msg, "equal Q-values must take the first maximum")
                    am = np.zeros(batch, np.int64)
                else:
                    am = np.argmax(qn, axis=1)
                    # an fp32 argmax may differ from the fp64 one only where two values are closer than their bounds
                    gap_ok = qn[b, am] - qn[b, oam] <= en[b, am] + en[b, oam]
                    assert gap_ok.all(), (msg, c)
                    am = oam.astype(np.int64)
                tq = gamma * qt[b, am] * (1.0 - done)
                y64 = r + tq
                ey = gamma * et[b, am] * (1.0 - done) + 3 * U * np.abs(tq) + U * np.abs(y64)
                assert (np.abs(y[c] - y64) <= ey).all(), (msg, c)


# ---------------------------------------------------------------------------------------------------------------
# lenv_rn_shape_rows: the 64-lane stride over hidden units up to 256, input width up to 64, one wave per row
# ---------------------------------------------------------------------------------------------------------------
RN_S, RN_INFO = 47, 17              # the info types see exactly 64 inputs
RN_TYPES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 101, 102)
# largest |oracle - fp64| of the shaped reward over the LayerNorm configurations of one hidden size, measured on the CPU
LN_MEASURED_RN = {63: 6.10e-07, 64: 6.36e-07, 65: 1.31e-06, 128: 8.44e-07, 256: 1.48e-06}


def rn_rows(H):
    """53 distinct transitions; the 1 000-row launch repeats them (1000 = 18 * 53 + 46), so every block reads its own row index
    while the references stay 53 rows long."""
    rng = np.random.RandomState(8000 + H)
    s = rng.uniform(-1.5, 1.5, (53, RN_S)).astype(np.float32)
    s2 = rng.uniform(-1.5, 1.5, (53, RN_S)).astype(np.float32)
    info = rng.uniform(-1.5, 1.5, (53, RN_INFO)).astype(np.float32)
    r = rng.uniform(-2, 2, 53).astype(np.float32)
    return s, s2, info, r


def rn_shape64(t, gamma, L, H, act, ln, theta, s, s2, info, r):
    """(shaped, bound) of RewardEnv._calc_reward in fp64 (reference envs/reward_env.py:68-133)."""
    r = r.astype(np.float64)
    g = float(np.float32(gamma))
    if t == 0:
        return r, np.zeros(r.shape)
    if t > 100:
        lin = info.astype(np.float64) @ theta.astype(np.float64)
        e = RN_INFO * U * (np.abs(info.astype(np.float64)) @ np.abs(theta.astype(np.float64)))
        return (lin, e) if t == 101 else (r + lin, e + U * np.abs(r + lin))
    with_info = t in (3, 4, 7, 8)
    D = RN_S + RN_INFO if with_info else RN_S
    x1 = np.concatenate([s, info], axis=1) if with_info else s
    x2 = np.concatenate([s2, info], axis=1) if with_info else s2
    p1, e1 = fwd64(D, H, L, 1, act, ln, theta, x1)
    p2, e2 = fwd64(D, H, L, 1, act, ln, theta, x2)
    p1, e1, p2, e2 = p1[:, 0], e1[:, 0], p2[:, 0], e2[:, 0]
    if t in (1, 3):
        y = g * p2 - p1
        return y, g * e2 + e1 + U * np.abs(g * p2) + U * np.abs(y)
    if t in (2, 4):
        y = (r + g * p2) - p1
        return y, g * e2 + e1 + U * np.abs(g * p2) + U * np.abs(r + g * p2) + U * np.abs(y)
    if t in (5, 7):
        return p2, e2
    return r + p2, e2 + U * np.abs(r + p2)


@pytest.mark.parametrize("H", [63, 64, 65, 128, 256])
def test_rn_shape_rows_shapes(eng, orc, H):
    """All eleven reward types x layers 1-4 x LayerNorm on/off, with 1 and 1 000 rows."""
    gamma = 0.97
    s, s2, info, r = rn_rows(H)
    rep = np.arange(1000) % 53
    big = [dev(v[rep]) for v in (s, s2, info, r)]
    one = [dev(v[:1]) for v in (s, s2, info, r)]
    for L in (1, 2, 3, 4):
        for ln in (False, True):
            act = ACTS[(L + H + int(ln)) % 5]
            for t in RN_TYPES:
                msg = "type %d H %d layers %d ln %d %s" % (t, H, L, ln, act)
                with_info = t in (3, 4, 7, 8)
                D = RN_S + RN_INFO if with_info else RN_S
                rng = np.random.RandomState(8100 + 10 * L + int(ln) + 7 * t)
                desc = None
                if t == 0:
                    theta = None
                elif t > 100:
                    theta = rng.uniform(-1, 1, RN_INFO).astype(np.float32)
                else:
                    theta = make_params(rng, D, H, L, 1, ln and L >= 2)
                    desc = eng.mlp_desc(D, H, L, 1, act, PRELU, ln)
                    assert eng.mlp_num_params(desc) == theta.size
                want = orc.rn_shape_rows(t, RN_S, RN_INFO, H, L, act, PRELU, gamma, theta, s, s2, info, r, use_layer_norm=ln)
                y, e = rn_shape64(t, gamma, L, H, act, ln and L >= 2, theta, s, s2, info, r)
                d_theta = dev(theta) if theta is not None else None
                got = eng.rn_shape_rows(t, desc, RN_S, RN_INFO, gamma, d_theta, *big).cpu().numpy()
                assert np.array_equal(got, want[rep]), msg
                check_against_fp64(got, y[rep], e[rep], LN_MEASURED_RN.get(H, 0.0), msg)
                got1 = eng.rn_shape_rows(t, desc, RN_S, RN_INFO, gamma, d_theta, *one).cpu().numpy()
                assert np.array_equal(got1, want[:1]), msg


# ---------------------------------------------------------------------------------------------------------------
# lenv_se_step_population: 3 H units over 256 threads, n_per_chain rows per workgroup, theta staged in LDS
# ---------------------------------------------------------------------------------------------------------------
SE_A = 3
SE_LN_FLAGS = (False, True, False), (True, False, True)        # (state, reward, done) nets: the flags differ between the three
# largest |oracle - fp64| over the LayerNorm nets of one (H, S) case, measured on the CPU
LN_MEASURED_SE = {(85, 1): 3.99e-07, (85, 17): 7.12e-07, (86, 1): 6.46e-07, (86, 17): 7.47e-07}      # (H 128 with a second layer is refused)


def se_case(H, L, S, n_per_chain, flags, chains=7):
    rng = np.random.RandomState(9000 + 10 * H + L + 1000 * S + n_per_chain + int(flags[0]))
    K = S + SE_A
    outs = (S, 1, 1)
    nets = [make_params(rng, K, H, L, o, f and L >= 2) for o, f in zip(outs, flags)]
    theta = np.concatenate(nets)
    pop = 3
    eps = (rng.randn(pop, theta.size) * 0.05).astype(np.float32)
    worker = rng.randint(0, pop, chains).astype(np.int32)
    worker[-1] = pop - 1
    sign = np.array([0.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0], np.float32)[:chains]
    state = rng.uniform(-1.5, 1.5, (chains, n_per_chain, S)).astype(np.float32)
    action = rng.randint(0, SE_A, (chains, n_per_chain)).astype(np.int32)
    return [n.size for n in nets], theta, eps, worker, sign, state, action


def se_lds_bytes(P, K, H):
    return 4 * (((P + 3) & ~3) + ((K + 3) & ~3) + 6 * H + 16)


@pytest.mark.parametrize("S", [1, 17, 200])
@pytest.mark.parametrize("H", [85, 86, 128])
def test_se_step_population_shapes(eng, orc, H, S):
    """Layers 1-3 x n_per_chain {1, 5} x two assignments of LayerNorm to the three nets, 7 chains of perturbed weights
    W_c = fma(sign[c], eps[worker[c]], theta).  A theta that does not fit the 160 KiB of LDS beside the activations is refused on
    the host with LENV_ERR_UNSUPPORTED (nothing is launched); the wide cases here reach that."""
    K = S + SE_A
    ran = refused = 0
    for L in (1, 2, 3):
        for n_per_chain in (1, 5):
            for flags in SE_LN_FLAGS:
                msg = "H %d layers %d S %d n %d ln %s" % (H, L, S, n_per_chain, flags)
                act = ACTS[(H + L + S + n_per_chain) % 5]
                sizes, theta, eps, worker, sign, state, action = se_case(H, L, S, n_per_chain, flags)
                descs = tuple(eng.mlp_desc(K, H, L, o, act, PRELU, f) for o, f in zip((S, 1, 1), flags))
                assert [eng.mlp_num_params(d) for d in descs] == sizes, msg
                args = (descs, dev(theta), dev(eps), dev(worker), dev(sign), dev(state), dev(action))
                assert 4 * theta.size > 160 * 1024 or se_lds_bytes(theta.size, K, H) <= 160 * 1024, msg     # no case sits in between
                if 4 * theta.size > 160 * 1024:
                    with pytest.raises(NotImplementedError, match=r"\(-2\)"):       # LENV_ERR_UNSUPPORTED
                        eng.se_step_population(*args)
                    refused += 1
                    continue
                ran += 1
                ns, r, d = [v.cpu().numpy() for v in eng.se_step_population(*args)]
                chains = state.shape[0]
                odescs = tuple(orc.mlp_desc(K, H, L, o, act, PRELU, f) for o, f in zip((S, 1, 1), flags))
                rep = np.repeat(np.arange(chains), n_per_chain)
                ons, orr, od = orc.se_step_population(odescs, theta, eps, worker[rep], sign[rep], state.reshape(-1, S), action.reshape(-1))
                assert np.array_equal(ns.reshape(-1, S), ons) and np.array_equal(r.reshape(-1), orr) and np.array_equal(d.reshape(-1), od), msg
                off = 0
                for size, o, f, got in zip(sizes, (S, 1, 1), flags, (ns, r, d)):
                    for c in range(chains):
                        w = (np.float32(sign[c]) * eps[worker[c], off:off + size] + theta[off:off + size]).astype(np.float32)
                        # fma(sign, eps, theta) with sign in {0, +-1}: the product is exact, so the sum above rounds once like the fma
                        x = np.concatenate([np.eye(SE_A, dtype=np.float32)[action[c]], state[c]], axis=1)
                        y, e = fwd64(K, H, L, o, act, f and L >= 2, w, x)
                        check_against_fp64(got[c].reshape(n_per_chain, o), y, e, LN_MEASURED_SE.get((H, S), 0.0), msg)
                    off += size
    assert ran + refused == 12 and (ran == 0) == (S == 200) and (S < 200 or refused == 12), (ran, refused)


# ---------------------------------------------------------------------------------------------------------------
# batched real envs: lenv_real_env_*, lenv_cont_env_*, lenv_cheetah_standin_* for n instances
# ---------------------------------------------------------------------------------------------------------------
PI = 3.141592653589793
STREAM_TEST_RESET = 4
MAX_STEPS = 200
#            id, fp64 state words, observation width, action width (0: a discrete index), number of actions
ENV_SPECS = {"cartpole": (0, 4, 4, 0, 2), "acrobot": (1, 4, 6, 0, 3), "mountaincar": (3, 4, 2, 0, 3),
             "cheetah": (2, 17, 17, 6, 0), "pendulum": (4, 2, 3, 1, 0), "cmc": (5, 2, 2, 1, 0)}


def env_states(name, n, rng):
    """(state [n, SD] fp64, action) over the whole state space; the first rows sit on the edges, then everything is shuffled so the
    edges land in any block."""
    _, SD, _, A, nA = ENV_SPECS[name]
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, -np.inf)
    if name == "cartpole":
        thr = 12 * 2 * PI / 360
        st = np.stack([rng.uniform(-2.6, 2.6, n), rng.uniform(-3, 3, n), rng.uniform(-0.25, 0.25, n), rng.uniform(-3, 3, n)], axis=1)
        edges = []
        for x in (2.4, up(2.4), -2.4, dn(-2.4)):                    # x_dot = 0: the new x is the old one, on / just past +-2.4
            edges.append([x, 0.0, 0.01, 0.3])
        for th in (thr, up(thr), -thr, dn(-thr)):                   # theta_dot = 0: the same for +-12 degrees
            edges.append([0.1, 0.2, th, 0.0])
    elif name == "acrobot":
        st = np.stack([rng.uniform(-PI, PI, n), rng.uniform(-PI, PI, n), rng.uniform(-4 * PI, 4 * PI, n), rng.uniform(-9 * PI, 9 * PI, n)], axis=1)
        edges = [[PI, 0.3, 4 * PI, 2.0], [-PI, -0.3, -4 * PI, -2.0],      # the +-pi wrap with the first velocity at its clip
                 [3.1, PI, 1.0, 9 * PI], [-3.1, -PI, -1.0, -9 * PI],      # second link at the wrap, second velocity at its clip
                 [PI / 2, 0.0, 0.0, 0.0], [2.0, 1.0, 0.5, -0.5],           # around the terminal line -cos(t1) - cos(t1 + t2) = 1
                 [2.0944, 0.0, 0.05, 0.0], [2.09, 0.01, 0.2, 0.1]]
    elif name in ("mountaincar", "cmc"):
        flag = 0.5 if name == "mountaincar" else 0.45
        st = np.zeros((n, SD))
        st[:, 0], st[:, 1] = rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)
        edges = [[-1.2, -0.07], [-1.199, -0.07], [-1.2, 0.0],                   # the left wall: position clipped, velocity zeroed
                 [0.0, 0.07], [0.0, -0.07], [0.3, 0.0699],                       # the speed clip
                 [flag - 0.03, 0.03], [flag - 0.0301, 0.03], [flag, 0.0], [flag, -0.001], [flag + 0.05, 0.002], [0.6, 0.07]]   # the flag
        edges = [e + [0.0] * (SD - 2) for e in edges]
    elif name == "pendulum":
        st = np.stack([rng.uniform(-100, 100, n), rng.uniform(-8, 8, n)], axis=1)
        edges = [[0.3, 8.0], [-0.3, -8.0], [100.0, 7.9], [-100.0, -7.9], [PI, 0.0], [-PI, 0.0], [0.0, 0.0]]
    else:
        st = rng.uniform(-10, 10, (n, 17))
        edges = [np.full(17, 10.0), np.full(17, -10.0), np.where(np.arange(17) % 2, 10.0, -10.0)]
    edges = np.array(edges, np.float64)[:n]
    st[:edges.shape[0]] = edges
    if A == 0:
        action = rng.randint(0, nA, n).astype(np.int32)
    elif name == "pendulum":
        action = rng.uniform(-3, 3, (n, 1)).astype(np.float32)                  # torques beyond +-2
        action[:min(n, 4), 0] = np.array([2.5, -2.5, 2.0, -2.0], np.float32)[:min(n, 4)]
    else:
        action = rng.uniform(-1.5, 1.5, (n, A)).astype(np.float32)              # beyond the +-1 of the force clip
    elapsed = rng.randint(0, MAX_STEPS - 1, n).astype(np.int32)
    elapsed[::5] = MAX_STEPS - 1                                                # TimeLimit fires on this step
    elapsed[1::5] = MAX_STEPS - 2
    perm = rng.permutation(n)
    return st[perm], action[perm], elapsed[perm]


def oracle_env_step(L, name, st, action):
    """One instance through the oracle's step function: (new state, fp32 obs, fp32 reward, env's own done)."""
    SD = st.size
    x = (C.c_double * SD)(*st)
    rew, done = C.c_double(0.0), C.c_int(0)
    if name in ("cartpole", "acrobot", "mountaincar"):
        getattr(L, "orc_%s_step" % name)(x, C.c_int(int(action)), C.byref(rew), C.byref(done))
    else:
        a = (C.c_float * action.size)(*action)
        if name == "cheetah":
            L.orc_cheetah_step(x, a, C.byref(rew))
        elif name == "pendulum":
            L.orc_pendulum_step(x, a, C.byref(rew))
        else:
            L.orc_cmc_step(x, a, C.byref(rew), C.byref(done))
    new = np.array(x[:], np.float64)
    if name == "acrobot":
        o = (C.c_double * 6)()
        L.orc_acrobot_obs(x, o)
        obs = np.array(o[:], np.float64)
    elif name == "pendulum":
        obs = np.array([L.orc_cos(new[0]), L.orc_sin(new[0]), new[1]])
    else:
        obs = new[:ENV_SPECS[name][2]]
    return new, obs.astype(np.float32), np.float32(rew.value), done.value


def reset_reference(L_hip, name, key, episode):
    """The reset draw from the host function lenv_rng_unit in numpy fp64 arithmetic (gym's np_random.uniform(low, high) per env)."""
    u = lambda i: np.float64(L_hip.lenv_rng_unit(key, STREAM_TEST_RESET, i))
    if name == "cartpole":
        return np.array([np.float64(-0.05) + np.float64(2 * 0.05) * u(episode * 4 + i) for i in range(4)])
    if name == "acrobot":
        return np.array([np.float64(-0.1) + np.float64(2 * 0.1) * u(episode * 4 + i) for i in range(4)])
    if name == "mountaincar":
        return np.array([np.float64(-0.6) + np.float64(0.2) * u(episode * 4), 0.0, 0.0, 0.0])
    if name == "cmc":
        return np.array([np.float64(-0.6) + np.float64(0.2) * u(episode * 2), 0.0])
    if name == "pendulum":
        return np.array([np.float64(-PI) + np.float64(2 * PI) * u(episode * 2), np.float64(-1.0) + np.float64(2.0) * u(episode * 2 + 1)])
    return np.array([np.float64(-0.1) + np.float64(0.2) * u(episode * 17 + i) for i in range(17)])


def env_obs_of(L, name, st):
    if name == "acrobot":
        return np.array([L.orc_cos(st[0]), L.orc_sin(st[0]), L.orc_cos(st[1]), L.orc_sin(st[1]), st[2], st[3]]).astype(np.float32)
    if name == "pendulum":
        return np.array([L.orc_cos(st[0]), L.orc_sin(st[0]), st[1]]).astype(np.float32)
    return st[:ENV_SPECS[name][2]].astype(np.float32)


def env_entry_points(L_hip, name):
    """[(reset, step)] closures over the raw C entry points serving `name` (the stand-in has its own pair beside lenv_cont_env_*)."""
    env_id = ENV_SPECS[name][0]
    if name in ("cartpole", "acrobot", "mountaincar"):
        return [(lambda *a: L_hip.lenv_real_env_reset(env_id, *a), lambda *a: L_hip.lenv_real_env_step(env_id, MAX_STEPS, *a))]
    pairs = [(lambda *a: L_hip.lenv_cont_env_reset(env_id, *a), lambda *a: L_hip.lenv_cont_env_step(env_id, MAX_STEPS, *a))]
    if name == "cheetah":
        pairs.append((lambda *a: L_hip.lenv_cheetah_standin_reset(*a), lambda *a: L_hip.lenv_cheetah_standin_step(MAX_STEPS, *a)))
    return pairs


@pytest.mark.parametrize("name", sorted(ENV_SPECS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_batched_envs(eng, orc, n, name):
    """n instances through the raw entry points: every instance's fp64 state, fp32 observation, reward, done flag and TimeLimit
    counter equal the oracle's step function on that instance; resets equal gym's uniform draw computed in numpy from
    lenv_rng_unit."""
    from learning_environments_amd import _lib
    L_hip, L = _lib.lib(), orc.lib()
    for f in ("orc_cartpole_step", "orc_acrobot_step", "orc_mountaincar_step", "orc_cheetah_step", "orc_pendulum_step", "orc_cmc_step",
              "orc_acrobot_obs"):
        getattr(L, f).restype = None
    _, SD, S, A, _ = ENV_SPECS[name]
    rng = np.random.RandomState(600 + n + 17 * ENV_SPECS[name][0])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for reset, step in env_entry_points(L_hip, name):
        # reset
        keys = rng.randint(0, 2 ** 63 - 1, n, dtype=np.int64)
        episode = rng.randint(0, 5000, n).astype(np.int64)
        d_state = torch.full((n, SD), 99.0, dtype=torch.float64, device="cuda")
        d_obs = torch.full((n, S), 99.0, dtype=torch.float32, device="cuda")
        d_el = torch.full((n,), 99, dtype=torch.int32, device="cuda")
        d_keys, d_episode = dev(keys), dev(episode)
        _lib.check(reset(ptr(d_keys), ptr(d_episode), n, ptr(d_state), ptr(d_obs), ptr(d_el), eng._stream()), "reset")
        g_state, g_obs = d_state.cpu().numpy(), d_obs.cpu().numpy()
        assert not d_el.cpu().numpy().any()
        for i in range(n):
            want = reset_reference(L_hip, name, int(keys[i]), int(episode[i]))
            assert np.array_equal(g_state[i], want), (name, n, i)
            assert np.array_equal(g_obs[i], env_obs_of(L, name, want)), (name, n, i)
        # step
        st, action, elapsed = env_states(name, n, rng)
        d_state, d_el, d_action = dev(st), dev(elapsed), dev(action)
        d_obs = torch.full((n, S), 99.0, dtype=torch.float32, device="cuda")
        d_rew = torch.full((n,), 99.0, dtype=torch.float32, device="cuda")
        d_done = torch.full((n,), 99.0, dtype=torch.float32, device="cuda")
        _lib.check(step(n, ptr(d_action), ptr(d_state), ptr(d_el), ptr(d_obs), ptr(d_rew), ptr(d_done), eng._stream()), "step")
        g_state, g_obs, g_rew, g_done, g_el = [t.cpu().numpy() for t in (d_state, d_obs, d_rew, d_done, d_el)]
        assert np.array_equal(g_el, elapsed + 1)
        env_done = 0
        for i in range(n):
            new, obs, rew, done = oracle_env_step(L, name, st[i], action[i])
            env_done += done
            assert np.array_equal(g_state[i], new), (name, n, i, st[i], g_state[i], new)
            assert np.array_equal(g_obs[i], obs), (name, n, i)
            assert g_rew[i] == rew, (name, n, i)
            assert g_done[i] == (1.0 if done or elapsed[i] + 1 >= MAX_STEPS else 0.0), (name, n, i)
        if n >= 255:                                         # the samples do reach the terminal conditions, and do not only reach them
            assert (g_done == 1.0).any() and (g_done == 0.0).any()
            if name in ("cartpole", "acrobot", "mountaincar", "cmc"):
                assert 0 < env_done < n


def test_pendulum_observation_cos_sin(eng, orc):
    """A grid of 1 000 angles over +-100 rad through one Pendulum step: the observation's cos / sin of the NEW angle (the fp64 state
    the kernel wrote) lie within one fp32 spacing of np.cos / np.sin."""
    from learning_environments_amd import _lib
    L_hip = _lib.lib()
    n = 1000
    st = np.stack([np.linspace(-100.0, 100.0, n), np.zeros(n)], axis=1)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    d_state, d_el, d_action = dev(st), dev(np.zeros(n, np.int32)), dev(np.zeros((n, 1), np.float32))
    d_obs = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    d_rew, d_done = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    _lib.check(L_hip.lenv_cont_env_step(4, MAX_STEPS, n, ptr(d_action), ptr(d_state), ptr(d_el), ptr(d_obs), ptr(d_rew),
                                        ptr(d_done), eng._stream()), "step")
    th, obs = d_state.cpu().numpy()[:, 0], d_obs.cpu().numpy().astype(np.float64)
    assert np.abs(th - st[:, 0]).max() > 1e-3                  # the step moved the angles off the grid
    for got, ref in ((obs[:, 0], np.cos(th)), (obs[:, 1], np.sin(th))):
        assert (np.abs(got - ref) <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).all()
