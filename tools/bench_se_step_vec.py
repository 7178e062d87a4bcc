"""One population step of a continuous-action synthetic env: lenv_se_step_population_vec (one launch for every chain) against the only
composition the tree offered before it -- per chain, W_c = theta + sign[c] * eps[worker[c]] on the host's stream and three lenv_mlp_forward
launches on cat(action, state).  Shapes: the published HalfCheetah SE 23-128-128-128-x (streaming kernel) and the MountainCarContinuous
SE 3-96-96-x (weights resident in LDS); 192 chains over 64 noise rows, n_per_chain 1 and 256, repeat 1.  Each figure: the median of 7
launches that end in a device synchronise, the two sides alternating; both sides' outputs are compared bit for bit first.
usage: python tools/bench_se_step_vec.py [chains]      (prints one JSON line per case; docs/notebook_se_step_vec.md holds a run)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning_environments_amd import engine      # noqa: E402

SHAPES = {"halfcheetah_23-128x3": (17, 6, 128, 3, "relu"), "cmc_3-96x2": (2, 1, 96, 2, "leakyrelu")}
REPS = 7


def composition(descs, sizes, theta, eps, worker, sign, x):
    """chains x (one perturbation + three forwards); x [chains, n, K]"""
    outs = []
    for c in range(x.shape[0]):                              # worker / sign: host lists, so that no step waits for the device
        w = theta + sign[c] * eps[worker[c]]
        outs.append([engine.mlp_forward(d, p.contiguous(), x[c]) for d, p in zip(descs, torch.split(w, sizes))])
    return [torch.stack([o[i] for o in outs]) for i in range(3)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    chains = int(sys.argv[1]) if len(sys.argv) > 1 else 192
    dev = engine.require_device()
    rng = np.random.RandomState(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for name, (S, A, H, L, act) in SHAPES.items():
        descs = engine.se_descs(S, A, H, L, act)
        sizes = [engine.mlp_num_params(d) for d in descs]
        P = sum(sizes)
        pop = chains // 3
        theta, eps = t((rng.randn(P) * 0.08).astype(np.float32)), t((rng.randn(pop, P) * 0.02).astype(np.float32))
        worker_h, sign_h = np.repeat(np.arange(pop), 3).tolist(), np.tile([0.0, 1.0, -1.0], pop).tolist()
        worker, sign = t(np.array(worker_h, np.int32)), t(np.array(sign_h, np.float32))
        for n in (1, 256):
            st, ac = t(rng.randn(chains, n, S).astype(np.float32)), t(rng.uniform(-1, 1, (chains, n, A)).astype(np.float32))
            x = torch.cat([ac, st], dim=2).contiguous()
            new = lambda: engine.se_step_population_vec(descs, theta, eps, worker, sign, st, ac)
            old = lambda: composition(descs, sizes, theta, eps, worker_h, sign_h, x)
            got, want = new(), old()                         # warm-up of both sides, and the same bits (sign in {-1, 0, 1})
            same = all(torch.equal(g.reshape(w.shape), w) for g, w in zip(got, want))
            t_new, t_old = [], []
            for _ in range(REPS):
                t_new.append(timed(new))
                t_old.append(timed(old))
            m_new, m_old = statistics.median(t_new), statistics.median(t_old)
            print(json.dumps({"shape": name, "params": P, "path": engine.se_step_vec_path(descs, n), "chains": chains, "n_per_chain": n,
                              "same_bits": same, "vec_ms": round(m_new * 1e3, 4), "composition_ms": round(m_old * 1e3, 4),
                              "composition_over_vec": round(m_old / m_new, 2), "vec_ms_min_max": [round(min(t_new) * 1e3, 4), round(max(t_new) * 1e3, 4)],
                              "composition_ms_min_max": [round(min(t_old) * 1e3, 4), round(max(t_old) * 1e3, 4)]}), flush=True)


if __name__ == "__main__":
    main()
