"""experiments/transfer_common.py on the CPU: the (theta, eps, worker, sign) of one and of several models, the per-model results and the
chain keys, as the four transfer drivers built them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from learning_environments_amd.agents.nes_common import chain_keys  # noqa: E402
from learning_environments_amd.experiments import transfer_common as tc  # noqa: E402

CPU = torch.device("cpu")
N_AG, P = 2, 5
MODELS = [torch.tensor([0.5, -0.0, 1.25, -3.0, 0.0]), torch.tensor([1.0, 2.0, -0.0, 4.0, 5.0]), torch.tensor([-1.5, 0.0, 7.0, -0.0, 9.0])]


def _bits(t):
    return t.contiguous().numpy().tobytes()


def _check_single(theta, eps, worker, sign, want_theta):
    assert theta.dtype == torch.float32 and _bits(theta) == _bits(want_theta)
    assert eps.dtype == torch.float32 and tuple(eps.shape) == (1, P) and not eps.any()
    assert worker.dtype == torch.int32 and worker.tolist() == [0] * N_AG
    assert sign.dtype == torch.float32 and sign.tolist() == [0.0] * N_AG


def test_one_model_and_no_model():
    def never():
        raise AssertionError("the other models are not asked for")
    _check_single(*tc.models_as_population(MODELS[0].double(), never, N_AG, N_AG, P, CPU), MODELS[0])
    _check_single(*tc.models_as_population(None, never, N_AG, N_AG, P, CPU), torch.zeros(P))
    # no model, several repetitions (the real env): still one zero theta, worker and sign 0 for every chain
    theta, eps, worker, sign = tc.models_as_population(None, never, 3 * N_AG, N_AG, P, CPU)
    assert _bits(theta) == _bits(torch.zeros(P)) and tuple(eps.shape) == (1, P) and not eps.any()
    assert worker.tolist() == [0] * 6 and sign.tolist() == [0.0] * 6


@pytest.mark.parametrize("others", [MODELS[1:], lambda: MODELS[1:]], ids=["list", "callable"])
def test_three_models(others):
    theta, eps, worker, sign = tc.models_as_population(MODELS[0], others, 3 * N_AG, N_AG, P, CPU)
    assert eps.dtype == torch.float32 and tuple(eps.shape) == (3, P)
    for m in range(3):
        assert _bits(eps[m]) == _bits(MODELS[m]), m                          # bit for bit: a stored -0.0 stays -0.0
    assert theta.dtype == torch.float32 and tuple(theta.shape) == (P,) and _bits(theta) == _bits(torch.zeros(P))
    assert worker.dtype == torch.int32 and worker.tolist() == [0, 0, 1, 1, 2, 2]
    assert sign.dtype == torch.float32 and sign.tolist() == [1.0] * 6


def test_a_model_of_another_size():
    with pytest.raises(ValueError, match="the models of one launch must have the same shapes"):
        tc.models_as_population(MODELS[0], [MODELS[1], torch.zeros(P + 1)], 3 * N_AG, N_AG, P, CPU)


def test_results_per_model():
    stats = np.zeros((4, 4), np.int64)
    stats[:, 0] = [2, 0, 3, 1]
    mean = np.arange(12, dtype=np.float64).reshape(4, 3) + 0.5
    lens = np.arange(12, dtype=np.int32).reshape(4, 3) + 100
    got = tc.results_per_model(stats, mean, lens, N_AG)
    assert got == [([[0.5, 1.5], []], [[100, 101], []]), ([[6.5, 7.5, 8.5], [9.5]], [[106, 107, 108], [109]])]


def test_model_chain_keys():
    seed, indices = 9, [4, 1]
    keys, keys_t = tc.model_chain_keys(seed, indices, N_AG, CPU)
    want = np.concatenate([chain_keys(seed, mi, np.arange(N_AG), np.zeros(N_AG, np.int64)) for mi in indices])
    assert keys.dtype == np.uint64 and np.array_equal(keys, want) and len(set(keys.tolist())) == 2 * N_AG
    assert keys_t.dtype == torch.int64 and keys_t.device == CPU and np.array_equal(keys_t.numpy().view(np.uint64), want)


def test_one_script_default_for_every_driver():
    from learning_environments_amd.experiments import transfer_algo, transfer_cartpole, transfer_vary_hp
    for mod in (transfer_algo, transfer_cartpole, transfer_vary_hp):
        assert mod.SCRIPT_DEFAULT is tc.SCRIPT_DEFAULT
