"""tests/se_fit_ref.c, the CPU restatement of the supervised VirtualEnv fit, against torch (no GPU).

The reference has no fit code, so the restatement is held to torch autograd and torch.optim.Adam, and the kernel to the restatement
(tests/test_se_fit_gpu.py).  The yardstick of (a) and (b) is torch's OWN fp32 distance from its fp64 run at the same point; the bound is
4 x that: two fp32 evaluations that differ only in summation order each sit about one such distance from fp64 and may sit on opposite sides
(x 2), doubled once more for outputs summed in a different association (and, over Adam steps, for the quotient while v is small).
Measured (docs/notebook_se_fit.md), max abs: (a) gradient yardstick 1.5e-8 / 3.4e-8 / 1.2e-8 (state / reward / done net), distance
1.5e-8 / 4.0e-8 / 1.1e-8; (b) parameters yardstick 1.4e-7, distance 1.4e-7, losses yardstick 1.8e-7, distance 4.3e-7; (c) 0 ulp."""
import numpy as np
import pytest
import torch

import se_fit_ref as ref

IN, S, H, L, ACT, B, N = 7, 5, 24, 2, "tanh", 20, 53


@pytest.fixture(scope="module")
def problem():
    torch.set_num_threads(1)
    rng = np.random.RandomState(11)
    ds = ref.descs(IN, S, H, L, ACT)
    theta = np.concatenate([rng.uniform(-1, 1, ref.net_params(d)).astype(np.float32) / np.sqrt(H) for d in ds])
    x = rng.randn(N, IN).astype(np.float32)
    y_state = rng.randn(N, S).astype(np.float32)
    y_reward = rng.randn(N).astype(np.float32)
    y_done = (rng.rand(N) < 0.3).astype(np.float32)
    tape = rng.randint(0, N, (100, B)).astype(np.int32)
    return dict(ds=ds, theta=theta, x=x, y=(y_state, y_reward, y_done), tape=tape)


def test_one_gradient_evaluation_sits_within_four_yardsticks_of_fp64_autograd(problem):
    p = problem
    rows, off = p["tape"][0], 0
    for d, y in zip(p["ds"], p["y"]):
        n = ref.net_params(d)
        prm, xb, yb = p["theta"][off:off + n], p["x"][rows], y.reshape(N, -1)[rows]
        off += n
        g64, l64 = ref.torch_grad(d, prm, xb, yb, torch.float64)
        g32, l32 = ref.torch_grad(d, prm, xb, yb, torch.float32)
        g, l = ref.grad(d, prm, xb, yb)
        yard, dist = np.abs(g32 - g64).max(), np.abs(g.astype(np.float64) - g64).max()
        print("grad out_dim %d: yardstick %.3g distance %.3g; loss yardstick %.3g distance %.3g" % (d.out_dim, yard, dist, abs(l32 - l64), abs(l - l64)))
        assert yard > 0.0 and dist <= 4.0 * yard
        assert abs(l - l64) <= 4.0 * max(abs(l32 - l64), np.spacing(np.float32(l64)))


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("act", ["identity", "relu", "leakyrelu", "tanh"])
def test_the_backward_of_every_admitted_activation_is_autograds(problem, act, layers):
    """(a) at each activation and depth the entry admits: the GPU cases compare the kernel with the restatement at relu, leakyrelu (slope
    0.01) and the identity too, so the restatement's act_bwd is anchored there as well.  Same yardstick, same bound."""
    p = problem
    rows, off = p["tape"][1], 0
    for d0, y in zip(p["ds"], p["y"]):
        d = ref.descs(IN, d0.out_dim, H, layers, act)[0]
        n = ref.net_params(d)
        prm, xb, yb = p["theta"][off:off + n], p["x"][rows], y.reshape(N, -1)[rows]
        off += ref.net_params(d0)
        g64, l64 = ref.torch_grad(d, prm, xb, yb, torch.float64)
        g32, l32 = ref.torch_grad(d, prm, xb, yb, torch.float32)
        g, l = ref.grad(d, prm, xb, yb)
        yard, dist = np.abs(g32 - g64).max(), np.abs(g.astype(np.float64) - g64).max()
        print("%s x %d out_dim %d: yardstick %.3g distance %.3g" % (act, layers, d.out_dim, yard, dist))
        assert np.abs(g64).max() > 1e-3 and yard > 0.0 and dist <= 4.0 * yard
        # the loss is ONE number, so torch's fp32 distance can be zero by accident and is no yardstick on its own: next to it stands the
        # worst-case error of a recursive fp32 sum of n = B * out_dim exact products (the fmaf chain), n * 2^-24 * sum / n = n * 2^-24 * loss
        n_terms = B * d.out_dim
        assert abs(l - l64) <= 4.0 * abs(l32 - l64) + n_terms * 2.0 ** -24 * l64


def test_a_hundred_adam_steps_stay_within_four_yardsticks_of_the_fp64_run(problem):
    p = problem
    t64, l64 = ref.torch_run(p["ds"], p["theta"], p["x"], *p["y"], p["tape"], torch.float64)
    t32, l32 = ref.torch_run(p["ds"], p["theta"], p["x"], *p["y"], p["tape"], torch.float32)
    out = ref.run(p["ds"], p["theta"], p["x"], *p["y"], B, len(p["tape"]), batch_idx=p["tape"][None])
    yard, dist = np.abs(t32 - t64).max(), np.abs(out["theta"][0].astype(np.float64) - t64).max()
    lyard, ldist = np.abs(l32 - l64).max(), np.abs(out["loss"][0].astype(np.float64) - l64).max()
    print("100 steps: theta yardstick %.3g distance %.3g; loss yardstick %.3g distance %.3g" % (yard, dist, lyard, ldist))
    assert l64[-10:].sum() < l64[:10].sum()                       # the fit does fit
    assert yard > 0.0 and dist <= 4.0 * yard
    assert lyard > 0.0 and ldist <= 4.0 * lyard


@pytest.mark.parametrize("step", [0, 1, 57])
def test_one_adam_step_on_given_gradients_equals_torch_to_one_ulp(step):
    rng = np.random.RandomState(step)
    n = 4096
    w = rng.randn(n).astype(np.float32)
    grads = [(rng.randn(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32) for _ in range(step + 1)]
    prm = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = torch.optim.Adam([prm], lr=1e-3)
    m, v, mine = np.zeros(n, np.float32), np.zeros(n, np.float32), w.copy()
    for t, g in enumerate(grads):
        if t == step:                                             # the step under test starts from torch's own state
            st = opt.state[prm]
            if t > 0:
                mine, m, v = prm.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
            mine, m, v = ref.adam(mine, m, v, g, t)
        prm.grad = torch.from_numpy(g.copy())
        opt.step()
    st = opt.state[prm]
    for name, got, want in (("param", mine, prm.detach().numpy()), ("exp_avg", m, st["exp_avg"].numpy()), ("exp_avg_sq", v, st["exp_avg_sq"].numpy())):
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))
        print("adam step %d %s: max %.2f ulp" % (step, name, ulps.max()))
        assert ulps.max() <= 1.0, name
