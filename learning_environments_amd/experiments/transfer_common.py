"""What the reward-net transfer drivers (transfer_gridworld / transfer_vary_hp / transfer_cartpole / transfer_algo) share: reading a
checkpoint, keying the chains, turning one or several models into the (theta, eps, worker, sign) of one launch, replaying recorded agents,
and collecting the per-model results.  Every helper takes the device as an argument."""
import numpy as np
import torch

from ..agents.nes_common import chain_keys
from ..envs.env_factory import EnvFactory

SCRIPT_DEFAULT = object()  # episodes_per_launch: the driver's DEFAULT_EPISODES_PER_LAUNCH (None instead: one launch from the first episode to the final test)


def load_envs_and_config(model_file, solved_reward):
    """solved_reward: the value the scripts raise it to, or a function of the env name that gives it"""
    save_dict = torch.load(model_file, map_location="cpu")
    config = save_dict['config']
    config['device'] = 'cpu'
    env_name = config['env_name']
    config['envs'][env_name]['solved_reward'] = solved_reward(env_name) if callable(solved_reward) else solved_reward
    env_factory = EnvFactory(config=config)
    reward_env = env_factory.generate_reward_env()
    reward_env.load_state_dict(save_dict['model'])
    real_env = env_factory.generate_real_env()
    return reward_env, real_env, config


def model_chain_keys(seed, model_indices, agents_num, dev):
    """(keys uint64 [M * agents_num], the same as a device int64 tensor): agent i of model index mi is worker i of generation mi"""
    n = int(agents_num)
    keys = np.concatenate([chain_keys(int(seed), int(mi), np.arange(n), np.zeros(n, np.int64)) for mi in model_indices])
    return keys, torch.from_numpy(keys.view(np.int64)).to(dev)


def models_as_population(theta, others, chains, agents_num, p_theta, dev):
    """(theta, eps, worker, sign) of a launch whose chains read M models, agents_num chains each.  theta: the first model's flat parameters or
    None (the real env); others: the flat parameters of models 1.., a list or a callable that returns it (asked only when there are several)."""
    M = chains // int(agents_num)
    if theta is None or M == 1:
        # the real env, or one model: its weights are theta itself, sign 0 (the unperturbed checkpoint)
        theta = torch.zeros(p_theta, dtype=torch.float32, device=dev) if theta is None else theta.to(device=dev, dtype=torch.float32)
        worker = torch.zeros(chains, dtype=torch.int32, device=dev)
        sign = torch.zeros(chains, dtype=torch.float32, device=dev)
        eps = torch.zeros((1, theta.numel()), dtype=torch.float32, device=dev)
    else:
        # several models: chain (m, i) reads 0 + 1 * weights[m] (exact; a stored -0.0 becomes +0.0, which no sum downstream can tell apart)
        thetas = [theta] + list(others() if callable(others) else others)
        if any(t.numel() != theta.numel() for t in thetas):
            raise ValueError("train_test_agents_models: the models of one launch must have the same shapes")
        eps = torch.stack([t.to(device=dev, dtype=torch.float32) for t in thetas])
        theta = torch.zeros_like(eps[0])
        worker = torch.arange(chains, dtype=torch.int32, device=dev) // int(agents_num)
        sign = torch.ones(chains, dtype=torch.float32, device=dev)
    return theta, eps, worker, sign


def replay_agents(inner, replay, agents_num, M, dev):
    """The recorded agents (and ICMs) of a replay instead of fresh ones: row i into chain (m, i) of every model m, zeros behind it."""
    for name, rows in (("agent_init", replay["agent_init"]), ("icm_init", replay.get("icm_init"))):
        if rows is not None and getattr(inner, name) is not None:
            buf = getattr(inner, name)
            buf.zero_()
            for i, r in enumerate(rows):
                for m in range(M):
                    buf[m * agents_num + i, :len(r)] = torch.as_tensor(np.asarray(r, np.float32)).to(dev)


def results_per_model(stats, episode_test_mean, episode_len, agents_num):
    """[(rewards, episode_lengths) per model] from the outputs of a launch (host arrays): every chain's rows cut at its episodes run"""
    chains, n = len(stats), int(agents_num)
    rewards = [episode_test_mean[i, :int(stats[i, 0])].tolist() for i in range(chains)]
    lengths = [episode_len[i, :int(stats[i, 0])].tolist() for i in range(chains)]
    return [(rewards[m:m + n], lengths[m:m + n]) for m in range(0, chains, n)]


def inner_results(inner, agents_num):
    """results_per_model of an inner loop that has run (synchronises)"""
    return results_per_model(inner.stats.cpu().numpy(), inner.episode_test_mean.cpu().numpy(), inner.episode_len.cpu().numpy(), agents_num)
