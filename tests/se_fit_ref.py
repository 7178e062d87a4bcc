"""Loader of tests/se_fit_ref.c, the CPU restatement of the supervised VirtualEnv fit (TEST INFRASTRUCTURE).

Compiled with the oracle Makefile's flags next to the oracle library, whose exported primitives (orc_mlp_forward, orc_rng_u64) it calls.  The
descs are the product's own ctypes mirror (learning_environments_amd._lib.MlpDesc, the layout of orc_mlp_desc), so one triple feeds the
kernel and the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np

from learning_environments_amd import _lib
from oracle import oracle as orc

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "se_fit_ref.c")
_OUT = os.path.join(os.path.dirname(_HERE), "oracle", "_build", "libse_fit_ref.so")
# oracle/Makefile's CFLAGS: -ffp-contract=off is what makes an FMA exist only where fmaf is written
CFLAGS = ["-O2", "-ffp-contract=off", "-mfma", "-fno-math-errno", "-fPIC", "-Wall", "-Wextra", "-std=c11"]

_ref = None
_D = C.POINTER(_lib.MlpDesc)
_F = C.POINTER(C.c_float)


def lib():
    global _ref
    if _ref is None:
        orc_path = orc.build()
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < os.path.getmtime(_SRC):
            subprocess.check_call([os.environ.get("CC", "gcc")] + CFLAGS + ["-shared", "-o", _OUT, _SRC, "-lm"])
        C.CDLL(orc_path, mode=C.RTLD_GLOBAL)          # the oracle's exported primitives resolve from it
        L = C.CDLL(_OUT)
        L.se_fit_ref_grad.restype = C.c_int
        L.se_fit_ref_grad.argtypes = [_D, _F, _F, _F, C.c_int32, _F, _F]
        L.se_fit_ref_adam.restype = None
        L.se_fit_ref_adam.argtypes = [_F, _F, _F, _F, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double]
        L.se_fit_ref_run.restype = C.c_int
        L.se_fit_ref_run.argtypes = [_D, _D, _D, _F, _F, _F, _F, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_int64, _F, _F, _F, _F]
        _ref = L
    return _ref


def descs(in_dim, S, hidden, layers, act):
    """(state, reward, done) descs of a VirtualEnv whose nets see in_dim inputs"""
    return tuple(_lib.MlpDesc(in_dim, hidden, layers, o, _lib.ACT[act] if isinstance(act, str) else act, 0.25, 0) for o in (S, 1, 1))


def net_params(d):
    return d.in_dim * d.hidden + d.hidden + (d.layers - 1) * (d.hidden * d.hidden + d.hidden) + d.hidden * d.out_dim + d.out_dim


def num_params(ds):
    return sum(net_params(d) for d in ds)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a, ct=C.c_float):
    return a.ctypes.data_as(C.POINTER(ct))


def grad(d, params, xb, yb):
    """(gradient [P], mean loss) of F.mse_loss(net(xb), yb) for one net"""
    p, xb, yb = _f32(params), _f32(xb).reshape(-1, d.in_dim), _f32(yb).reshape(-1, d.out_dim)
    assert p.size == net_params(d) and xb.shape[0] == yb.shape[0]
    g, loss = np.zeros(p.size, np.float32), np.zeros(1, np.float32)
    rc = lib().se_fit_ref_grad(C.byref(d), _fp(p), _fp(xb), _fp(yb), xb.shape[0], _fp(g), _fp(loss))
    assert rc == 0
    return g, float(loss[0])


def adam(p, m, v, g, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam step number `step` (0-based) on copies of p, m, v"""
    p, m, v, g = _f32(p).copy(), _f32(m).copy(), _f32(v).copy(), _f32(g)
    lib().se_fit_ref_adam(_fp(p), _fp(m), _fp(v), _fp(g), p.size, int(step), lr, betas[0], betas[1], eps)
    return p, m, v


def run(ds, theta, x, y_state, y_reward, y_done, batch_size, steps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, rng_keys=None, batch_idx=None,
        step_begin=0, adam_m=None, adam_v=None):
    """The whole fit with engine.se_fit_population's arguments on numpy arrays: dict(theta, adam_m, adam_v, loss)."""
    P = num_params(ds)
    th = _f32(theta).reshape(-1, P).copy()
    models = th.shape[0]
    m = np.zeros_like(th) if adam_m is None else _f32(adam_m).reshape(models, P).copy()
    v = np.zeros_like(th) if adam_v is None else _f32(adam_v).reshape(models, P).copy()
    x = _f32(x).reshape(-1, ds[0].in_dim)
    N = x.shape[0]
    ys, yr, yd = _f32(y_state).reshape(N, ds[0].out_dim), _f32(y_reward).reshape(N), _f32(y_done).reshape(N)
    loss = np.zeros((models, steps, 3), np.float32)
    keys = idx = None
    if rng_keys is not None:
        keys = np.ascontiguousarray(np.asarray(rng_keys).astype(np.uint64)).reshape(models)
    if batch_idx is not None:
        idx = np.ascontiguousarray(batch_idx, dtype=np.int32).reshape(models, steps, batch_size)
    rc = lib().se_fit_ref_run(C.byref(ds[0]), C.byref(ds[1]), C.byref(ds[2]), _fp(x), _fp(ys), _fp(yr), _fp(yd), N, batch_size, step_begin,
                              step_begin + steps, lr, betas[0], betas[1], eps, _fp(keys, C.c_uint64) if keys is not None else None,
                              _fp(idx, C.c_int32) if idx is not None else None, models, _fp(th), _fp(m), _fp(v), _fp(loss))
    assert rc == 0
    return dict(theta=th, adam_m=m, adam_v=v, loss=loss)


def forward(d, params, x):
    return orc.mlp_forward(orc.mlp_desc(d.in_dim, d.hidden, d.layers, d.out_dim, d.act), _f32(params), _f32(x))


# ---- the same fit in torch (fp32 or fp64), for the CPU tests and the measurement tool ----

def torch_net(d, params, dtype):
    """nn.Sequential of build_nn_from_config's shape with the flat parameter vector loaded"""
    import torch
    act = {0: torch.nn.Identity, 1: torch.nn.ReLU, 2: torch.nn.LeakyReLU, 3: torch.nn.Tanh}[d.act]
    mods, n_in = [], d.in_dim
    for _ in range(d.layers):
        mods += [torch.nn.Linear(n_in, d.hidden), act()]
        n_in = d.hidden
    mods.append(torch.nn.Linear(n_in, d.out_dim))
    net = torch.nn.Sequential(*mods).to(dtype)
    flat = torch.from_numpy(_f32(params)).to(dtype)
    off = 0
    with torch.no_grad():
        for prm in net.parameters():
            prm.copy_(flat[off:off + prm.numel()].reshape(prm.shape))
            off += prm.numel()
    assert off == flat.numel()
    return net


def torch_flat(net):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).double().numpy()


def torch_grad(d, params, xb, yb, dtype):
    """(gradient as float64 numpy, loss) by autograd in `dtype`"""
    import torch
    net = torch_net(d, params, dtype)
    xb = torch.from_numpy(_f32(xb).reshape(-1, d.in_dim)).to(dtype)
    yb = torch.from_numpy(_f32(yb).reshape(-1, d.out_dim)).to(dtype)
    loss = torch.nn.functional.mse_loss(net(xb), yb)
    loss.backward()
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()]).double().numpy(), float(loss.detach())


def torch_run(ds, theta, x, y_state, y_reward, y_done, batch_idx, dtype, lr=1e-3):
    """One model's fit on the index tape batch_idx [steps, batch] with torch.optim.Adam: (theta float64 [P], loss float64 [steps, 3])"""
    import torch
    x = torch.from_numpy(_f32(x).reshape(-1, ds[0].in_dim)).to(dtype)
    ys = [torch.from_numpy(_f32(y).reshape(x.shape[0], -1)).to(dtype) for y in (y_state, y_reward, y_done)]
    theta, off, nets = _f32(theta), 0, []
    for d in ds:
        nets.append(torch_net(d, theta[off:off + net_params(d)], dtype))
        off += net_params(d)
    opt = torch.optim.Adam([p for n in nets for p in n.parameters()], lr=lr)
    losses = np.zeros((len(batch_idx), 3))
    for t, rows in enumerate(np.asarray(batch_idx)):
        rows = torch.from_numpy(np.asarray(rows, dtype=np.int64))
        opt.zero_grad()
        ls = [torch.nn.functional.mse_loss(n(x[rows]), y[rows]) for n, y in zip(nets, ys)]
        sum(ls).backward()
        opt.step()
        losses[t] = [float(l.detach()) for l in ls]
    return np.concatenate([torch_flat(n) for n in nets]), losses
