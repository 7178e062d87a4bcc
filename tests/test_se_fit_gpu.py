"""lenv_se_fit_population on the GPU against its CPU restatement (tests/se_fit_ref.c, held to torch by tests/test_se_fit_reference.py): theta,
adam_m, adam_v and loss bit for bit, at the smallest shapes where the kernel can go wrong.

  A  every dimension 1 (one row, one hidden unit, one minibatch row)
  B  odd sizes, two hidden layers, tanh; counter mode, and a tape with a row repeated inside one batch
  C  the published CartPole SE 6-128-{4,1,1} (parameters, moments and gradient resident in LDS)
  D  the corner 32-128-128-32 at batch 256: four row chunks, parameters in the caller's arrays, gradient in the workspace
  E  a hidden width that is no multiple of the forward's four-unit items, identity activation
  F  a batch one chunk and a bit long (64 + 6 rows): the gradient chains continue over the chunk boundary"""
import ctypes as C

import numpy as np
import pytest
import torch

import se_fit_ref as ref
from learning_environments_amd import _lib, engine

pytestmark = pytest.mark.gpu

#            in   S    H  L  act          B    N   steps models mode
CASES = {
    "A": (3, 1, 1, 1, "relu", 1, 1, 3, 1, "counter"),
    "B_counter": (7, 5, 40, 2, "tanh", 20, 53, 12, 3, "counter"),
    "B_tape": (7, 5, 40, 2, "tanh", 20, 53, 12, 3, "tape_repeat"),
    "C": (6, 4, 128, 1, "leakyrelu", 64, 500, 8, 5, "counter"),
    "D": (32, 32, 128, 2, "relu", 256, 300, 2, 2, "tape"),
    "E": (5, 3, 33, 2, "identity", 7, 9, 4, 2, "tape"),
    "F": (4, 2, 16, 1, "tanh", 70, 31, 3, 2, "counter"),
}
_cache = {}


def problem(name):
    """the inputs of a case and the restatement's result (computed once, left unchanged)"""
    if name not in _cache:
        in_dim, S, H, L, act, B, N, steps, models, mode = CASES[name]
        rng = np.random.RandomState(sum(map(ord, name)))
        ds = ref.descs(in_dim, S, H, L, act)
        P = ref.num_params(ds)
        bounds = np.concatenate([np.concatenate([np.full(n_in * n_out + n_out, 1.0 / np.sqrt(n_in))
                                                 for n_in, n_out in [(in_dim, H)] + [(H, H)] * (L - 1) + [(H, d.out_dim)]]) for d in ds])
        assert bounds.size == P
        p = dict(ds=ds, B=B, steps=steps, models=models, P=P, N=N,
                 theta=(rng.uniform(-1, 1, (models, P)) * bounds).astype(np.float32),
                 x=rng.randn(N, in_dim).astype(np.float32), ys=rng.randn(N, S).astype(np.float32), yr=rng.randn(N).astype(np.float32),
                 yd=(rng.rand(N) < 0.3).astype(np.float32), keys=None, idx=None)
        if mode == "counter":
            p["keys"] = np.array([_lib.lib().lenv_chain_key(5, 0, m, 0) for m in range(models)], np.uint64)
        else:
            p["idx"] = rng.randint(0, N, (models, steps, B)).astype(np.int32)
            if mode == "tape_repeat":
                p["idx"][:, :, 3] = p["idx"][:, :, 11]
                p["idx"][0, 0, :] = 17
        p["ref"] = ref.run(ds, p["theta"], p["x"], p["ys"], p["yr"], p["yd"], B, steps, rng_keys=p["keys"], batch_idx=p["idx"])
        _cache[name] = p
    return _cache[name]


def dev(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def fit(p, steps=None, step_begin=0, theta=None, adam_m=None, adam_v=None, **kw):
    steps = p["steps"] if steps is None else steps
    idx = dev(p["idx"][:, step_begin:step_begin + steps]) if p["idx"] is not None else None
    out = engine.se_fit_population(p["ds"], dev(p["theta"]) if theta is None else theta, dev(p["x"]), dev(p["ys"]), dev(p["yr"]), dev(p["yd"]), p["B"],
                                   steps, rng_keys=dev(p["keys"]), batch_idx=idx, step_begin=step_begin, adam_m=adam_m, adam_v=adam_v, **kw)
    torch.cuda.synchronize()
    return out


def same_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %r != %r" % (what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_kernel_equals_the_restatement_bit_for_bit(name):
    p = problem(name)
    assert np.isfinite(p["ref"]["theta"]).all() and np.isfinite(p["ref"]["loss"]).all()
    assert not np.array_equal(p["ref"]["theta"], p["theta"])
    sn, rn, dn = p["ds"]
    ws = _lib.lib().lenv_se_fit_workspace_bytes(C.byref(sn), C.byref(rn), C.byref(dn), p["B"], p["models"])
    assert (ws > 0) == (name == "D")                                          # D alone takes the workspace path
    out = fit(p)
    for key in ("theta", "adam_m", "adam_v", "loss"):
        same_bits(out[key], p["ref"][key], "%s %s" % (name, key))


@pytest.mark.parametrize("name", ["B_counter", "B_tape"])
@pytest.mark.parametrize("split", ["5+7", "singles"])
def test_a_fit_resumed_with_its_moments_equals_the_fit_in_one_launch(name, split):
    p = problem(name)
    if split == "5+7":
        a = fit(p, steps=5)
        b = fit(p, steps=7, step_begin=5, theta=a["theta"], adam_m=a["adam_m"], adam_v=a["adam_v"])
        loss = torch.cat([a["loss"], b["loss"]], dim=1)
    else:
        b = fit(p, steps_per_launch=1)
        loss = b["loss"]
    for key, got in (("theta", b["theta"]), ("adam_m", b["adam_m"]), ("adam_v", b["adam_v"]), ("loss", loss)):
        same_bits(got, p["ref"][key], "%s %s %s" % (name, split, key))


def test_equal_keys_and_inits_give_equal_models_and_different_keys_different_ones():
    p = dict(problem("B_counter"))
    p["theta"] = np.repeat(p["theta"][:1], 3, axis=0)
    p["keys"] = np.array([p["keys"][0], p["keys"][1], p["keys"][0]], np.uint64)
    out = fit(p)
    theta, loss = out["theta"].cpu().numpy(), out["loss"].cpu().numpy()
    assert np.array_equal(theta[0], theta[2]) and np.array_equal(loss[0], loss[2])
    assert not np.array_equal(theta[0], theta[1]) and not np.array_equal(loss[0], loss[1])
    same_bits(theta[0], problem("B_counter")["ref"]["theta"][0], "model 0 does not depend on its neighbours")


@pytest.mark.parametrize("name", ["B_counter", "C", "D"])
def test_the_fitted_model_steps_through_lenv_mlp_forward_as_the_restatement_does(name):
    p = problem(name)
    theta = p["ref"]["theta"]
    x, off = dev(p["x"]), 0
    for d in p["ds"]:
        n = ref.net_params(d)
        for m in range(p["models"]):
            prm = np.ascontiguousarray(theta[m, off:off + n])
            got = engine.mlp_forward(engine.mlp_desc(d.in_dim, d.hidden, d.layers, d.out_dim, d.act), dev(prm), x)
            same_bits(got, ref.forward(d, prm, p["x"]).reshape(p["N"], d.out_dim), "%s forward out_dim %d model %d" % (name, d.out_dim, m))
        off += n


def test_the_python_entry_refuses_what_it_cannot_run():
    p = problem("A")
    t = dev(p["theta"])
    with pytest.raises(ValueError):
        engine.se_fit_population(p["ds"], t, dev(p["x"]), dev(p["ys"]), dev(p["yr"]), dev(p["yd"]), 1, 3)                       # neither keys nor tape
    with pytest.raises(ValueError):
        engine.se_fit_population(p["ds"], t, dev(p["x"]), dev(p["ys"]), dev(p["yr"]), dev(p["yd"]), 1, 3,
                                 batch_idx=torch.ones((1, 3, 1), dtype=torch.int32, device="cuda"))                             # row 1 of a 1-row data set
    with pytest.raises(NotImplementedError):
        engine.se_fit_population(ref.descs(3, 1, 1, 1, "prelu"), t, dev(p["x"]), dev(p["ys"]), dev(p["yr"]), dev(p["yd"]), 1, 3, rng_keys=dev(p["keys"]))
