"""The NES master step (csrc/nes_update.hip: draw, worker_best(_multi), status_fold, score_transform, update_env) at the sizes
where its loops take a second pass: populations across score_transform_kernel's 1 024-thread stride, theta lengths across
update_env_kernel's 256-wide blocks, a draw larger than nes_draw_kernel's capped grid of 4 096 x 256 threads.

Every case is held bit for bit against the CPU oracle AND against a second reference written here in plain numpy / python from the
reference's source (agents/GTN_master.py:197-298, agents/GTN_worker.py:234-254), so a slip shared by kernel and oracle shows too.
"""
import statistics

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_oracle_golden import g7p_cases, g7p_check_rank_type  # noqa: E402

pytestmark = pytest.mark.gpu


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
# second references, plain numpy / python
# ---------------------------------------------------------------------------------------------------------------
def np_score_transform(t, scores, scores_orig):
    """GTN_Master.score_transform restated line by line; ties rank in the project's documented order (lower worker id first)."""
    scores, scores_orig = np.array(scores, np.float64), np.asarray(scores_orig, np.float64)
    n = len(scores)
    if t == 0:
        return (scores - min(scores)) / (max(scores) - min(scores) + 1e-9)
    if t == 1:
        s = np.argsort(scores, kind="stable")
        out = np.zeros(n)
        for i in range(n):
            out[s[i]] = i / (n - 1)
        return out
    if t in (2, 3):
        s = np.argsort(-scores, kind="stable")
        out = np.zeros(n)
        for i in range(n):
            out[s[i]] = i + 1
        for i in range(n):
            out[i] = max(0, np.log(n / 2 + 1) - np.log(out[i]))
        out = out / sum(out)
        if t == 2:
            out -= 1 / n
        out /= max(out)
        return out
    if t == 4:
        out = np.zeros(n)
        out[np.argmax(scores)] = 1
        return out
    avg = np.mean(scores_orig)
    idx = np.where(scores > avg + 1e-6, 1, 0)
    if sum(idx) == 0:
        return idx.astype(np.float64)
    if t == 5:
        out = np.zeros(n)
        out[np.argmax(scores)] = 1
        return out
    out = idx * (scores - avg) / (max(scores) - avg + 1e-9)
    out /= max(out) if t == 6 else sum(out)
    return out


def np_update_env(theta, eps, sign, weights, step_size, nes_step_size, weight_decay):
    """GTN_Master.update_env on the flat theta: fp32 `theta * (1 - wd)`, then `theta + float32(ss * w) * (sign * eps)` in worker order."""
    ss = step_size / len(weights) if nes_step_size else step_size
    t = theta.astype(np.float32) * np.float32(1.0 - weight_decay)
    for w in range(len(weights)):
        t = t + np.float32(ss * weights[w]) * (np.float32(sign[w]) * eps[w])
    assert t.dtype == np.float32
    return t


def np_worker_best(add, sub, mirrored):
    best, sign = add.copy(), np.ones(add.size)
    if mirrored:
        flip = sub > add
        best[flip], sign[flip] = sub[flip], -1.0
    return best, sign


def gathered_of(scores, scores_orig, sign=None):
    g = np.zeros((len(scores), 4))
    g[:, 0], g[:, 1], g[:, 2] = scores, scores_orig, 1.0 if sign is None else sign
    return g


# ---------------------------------------------------------------------------------------------------------------
# score_transform against fixture G7P (the reference's own outputs)
# ---------------------------------------------------------------------------------------------------------------
def test_g7p_score_transform_kernel(eng, orc, golden):
    """score_transform_kernel on every case of fixture G7P: bit for bit the oracle's weights, and against the reference's under the
    rules of the CPU test (types 0 and 4-7 equal, types 1-3 at 1e-15, tie groups as for G7)."""
    from learning_environments_amd.agents.nes_common import rank_table
    g = golden("g7p_master_pops")
    tables = {}
    bad_oracle, bad_ref, n = [], [], 0
    for pop, name, t, sc, so, ref in g7p_cases(g):
        if (t, pop) not in tables:
            tables[(t, pop)] = dev(rank_table(t, pop))
        w = eng.nes_rank_update(t, dev(gathered_of(sc, so)), tables[(t, pop)], None, None, 0.0).cpu().numpy()
        n += 1
        if not np.array_equal(w, orc.score_transform(t, sc, so)):
            bad_oracle.append((pop, name, t))
        if t in (1, 2, 3):
            g7p_check_rank_type(w, ref, sc, "pop %d %s type %d" % (pop, name, t))
        elif not np.array_equal(w, ref):
            bad_ref.append((pop, name, t))
    assert n >= 9 * 5 * 8 - 7 * 3
    assert not bad_oracle, bad_oracle
    assert not bad_ref, bad_ref
    # update_env at pop 17 on a theta of 843 elements (three full blocks and a part)
    pop, P = g["u_eps"].shape
    gathered = dev(gathered_of(g["u_scores"], g["u_scores_orig"]))
    theta, eps = dev(g["u_theta0"].copy()), dev(g["u_eps"])
    w = eng.nes_rank_update(7, gathered, dev(rank_table(7, pop)), theta, eps, float(g["u_step_size"])).cpu().numpy()
    assert np.array_equal(w, g["u_weights"])
    assert np.array_equal(theta.cpu().numpy(), g["u_theta1"])
    eng.nes_rank_update(7, gathered, dev(rank_table(7, pop)), theta, eps, float(g["u_step_size"]), True, 0.01)
    assert np.array_equal(theta.cpu().numpy(), g["u_theta2"])


# ---------------------------------------------------------------------------------------------------------------
# nes_rank_update / _keep across the 1 024-thread stride and the 256-wide blocks
# ---------------------------------------------------------------------------------------------------------------
RANK_P = (1, 255, 256, 257, 1000)


def rank_update_inputs(pop):
    """Tie-free continuous scores (np.argsort's tie order is its own), mirrored signs, eps [pop, 1000] (the smaller P take its
    leading columns)."""
    rng = np.random.RandomState(4100 + pop)
    so = rng.normal(-300.0, 50.0, pop)
    sc = so + rng.normal(0.0, 20.0, pop)
    assert np.unique(sc).size == pop
    sign = np.where(rng.rand(pop) < 0.5, -1.0, 1.0)
    eps = (rng.randn(pop, max(RANK_P)) * 0.05).astype(np.float32)
    theta = (rng.randn(max(RANK_P)) * 0.3).astype(np.float32)
    return sc, so, sign, eps, theta


@pytest.mark.parametrize("pop", [2, 1023, 1024, 1025, 2500])
def test_rank_update_sizes(eng, orc, pop):
    """All eight types x P in {1, 255, 256, 257, 1000}: weights and the updated theta bit-equal to the oracle and to the numpy
    restatement; nes_step_size, weight_decay and the _keep form (theta_prev, generation counter) change with the type so that every
    combination of the three runs at every (pop, P)."""
    from learning_environments_amd.agents.nes_common import rank_table
    sc, so, sign, eps, theta0 = rank_update_inputs(pop)
    gathered = dev(gathered_of(sc, so, sign))
    step = 0.727
    for t in range(8):
        nes, wd, keep = bool(t & 1), (0.01 if t & 2 else 0.0), bool(t & 4)
        w_np = np_score_transform(t, sc, so)
        w_or = orc.score_transform(t, sc, so)
        assert np.array_equal(w_np, w_or), "type %d: the two references disagree" % t
        th_np = np_update_env(theta0, eps, sign, w_np, step, nes, wd)
        table = dev(rank_table(t, pop))
        for P in RANK_P:
            msg = "pop %d type %d P %d" % (pop, t, P)
            e = np.ascontiguousarray(eps[:, :P])
            theta = dev(theta0[:P].copy())
            if keep:
                prev, gen = torch.full((P,), 7.0, dtype=torch.float32, device="cuda"), dev(np.array([41], np.int64))
                w = eng.nes_rank_update(t, gathered, table, theta, dev(e), step, nes, wd, theta_prev=prev, generation=gen)
                assert np.array_equal(prev.cpu().numpy(), theta0[:P]), msg
                assert gen.cpu().tolist() == [42], msg
            else:
                w = eng.nes_rank_update(t, gathered, table, theta, dev(e), step, nes, wd)
            assert np.array_equal(w.cpu().numpy(), w_or), msg
            got = theta.cpu().numpy()
            assert np.array_equal(got, orc.update_env(theta0[:P], e, sign.astype(np.float32), w_or, step, nes, wd)), msg
            assert np.array_equal(got, th_np[:P]), msg


# ---------------------------------------------------------------------------------------------------------------
# nes_worker_best(_multi)
# ---------------------------------------------------------------------------------------------------------------
def worker_best_rows(pop, G):
    """chain_scores [pop, 1 + 2G]: returns within +-1e3, one entry in five a -1e9 time-out, every seventh worker with add == sub."""
    rng = np.random.RandomState(5200 + 31 * pop + G)
    cs = rng.uniform(-1e3, 1e3, (pop, 1 + 2 * G))
    cs[rng.rand(pop, 1 + 2 * G) < 0.2] = -1e9
    cs[::7, 1 + G:] = cs[::7, 1:1 + G]
    return cs


@pytest.mark.parametrize("pop", [1, 255, 256, 257, 1000])
def test_worker_best_sizes(eng, orc, pop):
    """calc_best_score for num_grad_evals G in {1, 2, 5, 16}, 'mean' and 'minmax', mirrored and not.  'mean' must be
    statistics.mean exactly for returns within +-1e3 mixed with -1e9 time-outs.  That is the promise: exact_mean carries the sum in
    two doubles (~106 bits), not exactly, so rows whose magnitudes are spread over many more decades than returns and time-outs are
    can come out one place away from statistics.mean.  Such rows are outside the promise and are not asserted here."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    for G in (1, 2, 5, 16):
        cs = worker_best_rows(pop, G)
        d_cs = dev(cs.reshape(-1))
        add, sub = cs[:, 1:1 + G], cs[:, 1 + G:]
        assert (add == sub).all(axis=1).any()
        exact = {"mean": (np.array([statistics.mean(r.tolist()) for r in add]), np.array([statistics.mean(r.tolist()) for r in sub])),
                 "minmax": (np.array([min(r.tolist()) for r in add]), np.array([min(r.tolist()) for r in sub]))}
        for kind in ("mean", "minmax"):
            for mirrored in (True, False):
                msg = "pop %d G %d %s mirrored %d" % (pop, G, kind, mirrored)
                res = eng.nes_worker_best(d_cs, pop, mirrored, G, kind).cpu().numpy()
                best, sign = np_worker_best(exact[kind][0], exact[kind][1], mirrored)
                assert np.array_equal(res[:, 0], best), msg
                assert np.array_equal(res[:, 1], cs[:, 0]), msg
                assert np.array_equal(res[:, 2], sign), msg
                assert not res[:, 3].any(), msg
                obest, osign = orc.worker_best_multi(add, sub, mirrored, kind)
                assert np.array_equal(res[:, 0], obest) and np.array_equal(res[:, 2], osign.astype(np.float64)), msg
                assert (res[::7, 2] == 1.0).all(), msg                          # add == sub keeps +eps
                if G == 1:
                    one = torch.full((pop, 4), -5.0, dtype=torch.float64, device="cuda")
                    _lib.check(L.lenv_nes_worker_best(d_cs.data_ptr(), pop, 1 if mirrored else 0, one.data_ptr(), eng._stream()), "lenv_nes_worker_best")
                    assert np.array_equal(one.cpu().numpy(), res), msg


# ---------------------------------------------------------------------------------------------------------------
# nes_status_fold
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 385, 5000])
def test_status_fold_minimum_in_the_last_slot(eng, n):
    pop = 6
    for last, want in ((-10, -10.0), (0, -3.0 if n > 1 else 0.0), (5, -3.0 if n > 1 else 0.0)):
        status = np.zeros(n, np.int32)
        if n > 1:
            status[n // 2] = -3
        status[-1] = last
        assert float(min(0, status.min())) == want
        result = dev(np.arange(pop * 4, dtype=np.float64).reshape(pop, 4))
        eng.nes_status_fold(dev(status), result)
        got = result.cpu().numpy()
        assert np.array_equal(got[:, :3], np.arange(pop * 4, dtype=np.float64).reshape(pop, 4)[:, :3])
        assert np.array_equal(got[:, 3], np.full(pop, want)), (n, last)


# ---------------------------------------------------------------------------------------------------------------
# nes_draw past the capped grid
# ---------------------------------------------------------------------------------------------------------------
def test_draw_wraps_the_grid(eng, orc):
    """pop * P = 5 * 209 801 = 1 049 005 noise elements, 15 x 401 agent parameters and 15 keys: 6 459 elements more than the
    4 096 x 256 threads of the capped grid, so the grid-stride loop takes a second pass that covers the tail of eps, every agent row
    and every key.  Bit-equal to the oracle's draw; the _dev entry (generation read on the device) gives the same tensors; 4 096
    sampled noise elements lie within one fp32 spacing of an fp64 Box-Muller computed in numpy from the host functions
    lenv_chain_key / lenv_rng_unit, scaled by noise_std in fp32 like the kernel does; agent rows and keys from the same functions."""
    from learning_environments_amd import _lib
    L = _lib.lib()
    seed, gen, pop, P, cpw, worker_lo, noise_std = 0x1234_5678_9abc, 3, 5, 209801, 3, 11, 0.0124
    chains = pop * cpw
    assert pop * P > 4096 * 256 and (pop - 1) * P < 4096 * 256
    rng = np.random.RandomState(9)
    bounds = rng.uniform(0.05, 0.5, 401).astype(np.float32)
    eps, init, keys = eng.nes_draw(seed, gen, pop, P, noise_std, chains, cpw, worker_lo, dev(bounds))
    eps2, init2, keys2 = eng.nes_draw(seed, dev(np.array([gen], np.int64)), pop, P, noise_std, chains, cpw, worker_lo, dev(bounds))
    assert torch.equal(eps, eps2) and torch.equal(init, init2) and torch.equal(keys, keys2)
    eps, init, keys = eps.cpu().numpy(), init.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
    oeps, oinit, okeys = orc.nes_draw(seed, gen, pop, P, noise_std, chains, cpw, worker_lo, bounds)
    assert np.array_equal(eps, oeps)
    assert np.array_equal(init, oinit)
    assert np.array_equal(keys, okeys)
    # keys and agent rows from the host functions
    STREAM_NES_EPS, STREAM_AGENT_INIT, EPS_DOMAIN = 9, 10, 0x6e65735f657073
    for c in range(chains):
        key = L.lenv_chain_key(seed, gen, worker_lo + c // cpw, c % cpw)
        assert int(keys[c]) == key
        u = np.array([L.lenv_rng_unit(key, STREAM_AGENT_INIT, i) for i in range(bounds.size)]).astype(np.float32)
        assert np.array_equal(init[c], (u * np.float32(2.0) - np.float32(1.0)) * bounds), c
    # fp64 Box-Muller on 4 096 elements: the first and last of every row, both sides of the grid's wrap, the rest at random
    edges = np.concatenate([np.arange(pop) * P, np.arange(pop) * P + P - 1, 4096 * 256 + np.arange(-2, 3)])
    flat = np.concatenate([edges, rng.choice(pop * P, 4096 - edges.size, replace=False)])
    ns32 = np.float32(noise_std)
    worst = 0.0
    for e in flat:
        w, i = divmod(int(e), P)
        key = L.lenv_chain_key(seed ^ EPS_DOMAIN, gen, w, 0)
        u1 = L.lenv_rng_unit(key, STREAM_NES_EPS, 2 * i) + 2.0 ** -53
        u2 = L.lenv_rng_unit(key, STREAM_NES_EPS, 2 * i + 1)
        z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
        zf = np.float32(z)
        near = [np.nextafter(zf, np.float32(-np.inf)), zf, np.nextafter(zf, np.float32(np.inf))]
        assert any(eps[w, i] == c * ns32 for c in near), (w, i, eps[w, i], z)
        worst = max(worst, abs(float(eps[w, i]) - z * float(ns32)) / float(np.spacing(np.float32(abs(z * float(ns32))))))
    print("nes_draw: worst distance from the fp64 Box-Muller over %d elements: %.3f fp32 spacings" % (flat.size, worst))
