"""EnvWrapper: the uniform tensor API over real / virtual envs (reference envs/env_wrapper.py:9-167).

Same methods, argument meaning and return conventions: `step(action, state=None)` returns the 3-tuple
`(next_state, reward, done)` of CPU fp32 tensors.  New (batched fast path, not in the reference):
`step_population` evaluates many NES perturbations of a virtual env, or of a reward env over a vector-state real env, in one kernel
launch.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib, engine
from ..utils import from_one_hot_encoding, to_one_hot_encoding
from .grid_env import GridEnv
from .reward_env import RewardEnv
from .spaces import Discrete
from .virtual_env import VirtualEnv


class PopulationState(object):
    """`chains` instances of a real env on the device, as lenv_real_env_step / lenv_cont_env_step keep them: state fp64 [chains,SD], elapsed
    int32 [chains] (steps of the running episode, for the TimeLimit) and obs fp32 [chains,S], the observation of `state`."""

    def __init__(self, state, elapsed, obs):
        self.state, self.elapsed, self.obs = state, elapsed, obs


class EnvWrapper(nn.Module):
    def __init__(self, env):
        super().__init__()
        self.env = env
        self.same_action_num = 1

    def step(self, action, state=None):
        if self.is_virtual_env():
            reward_sum = None
            if self.has_discrete_action_space():
                action = to_one_hot_encoding(action, self.get_action_dim())
            for _ in range(self.same_action_num):
                state, reward, done = self.env.step(action=action, state=state)
                reward_sum = reward if reward_sum is None else reward_sum + reward
            reward = reward_sum.to("cpu")
            next_state = state.to("cpu")
            done = done.to("cpu")
            if self.has_discrete_state_space():
                next_state = from_one_hot_encoding(next_state)
            return next_state, reward, done
        return self._step_real(action)

    def _step_real(self, action):
        """Real / reward env (reference :48-70): numpy action (an int for discrete spaces), the action repeated `same_action_num`
        times with summed rewards until the env reports done; 0-dim reward / done tensors, scalar states become 1-element
        vectors."""
        act = action.detach().cpu().numpy()
        if self.has_discrete_action_space():
            act = int(act.astype(int)[0])
        total, obs, done = 0, None, False
        for _ in range(self.same_action_num):
            obs, reward, done, _ = self.env.step(act)
            total += reward
            if done:
                break
        as_f32 = lambda v: torch.tensor(v, device="cpu", dtype=torch.float32)
        obs_t = as_f32(obs)
        return (obs_t.unsqueeze(0) if obs_t.dim() == 0 else obs_t), as_f32(total), as_f32(done)

    def _real_env(self):
        """The device-resident real env behind a non-virtual wrapper; a gridworld has no one-step population path (theirs is the QL kernel)."""
        real = self.env.real_env if isinstance(self.env, RewardEnv) else self.env
        if isinstance(real, GridEnv):
            raise NotImplementedError("step_population is not defined for a gridworld RewardEnv: its population path is the fused Q-learning kernel")
        return real

    def reset_population(self, chains, seed=0, episode=0):
        """Fresh episodes of `chains` independent instances of the real env behind a RewardEnv (or of the bare real env): chain c draws its
        reset state with the key lenv_chain_key(seed, 0, c, 3) -- chain 0 is the instance a DeviceRealEnv seeded with `seed` resets to at
        that episode.  Returns the PopulationState `step_population` advances."""
        if self.is_virtual_env():
            raise NotImplementedError("reset_population is defined for real and reward envs: a virtual env keeps no state of its own")
        real = self._real_env()
        dev = engine.require_device()
        L = _lib.lib()
        keys = np.array([L.lenv_chain_key(int(seed), 0, c, 3) for c in range(chains)], np.uint64).view(np.int64)
        keys = torch.from_numpy(keys).to(dev)
        ep = torch.full((chains,), int(episode), dtype=torch.int64, device=dev)
        S, SD, _ = engine.REAL_ENV_DIMS[real.env_id]
        st = PopulationState(torch.zeros((chains, SD), dtype=torch.float64, device=dev), torch.zeros(chains, dtype=torch.int32, device=dev),
                             torch.zeros((chains, S), dtype=torch.float32, device=dev))
        reset = L.lenv_cont_env_reset if real.continuous else L.lenv_real_env_reset
        _lib.check(reset(real.env_id, engine._ptr(keys), engine._ptr(ep), chains, engine._ptr(st.state), engine._ptr(st.obs),
                         engine._ptr(st.elapsed), engine._stream()), "lenv_real_env_reset")
        return st

    def step_population(self, actions, states, eps=None, worker=None, sign=None, repeat=1):
        """Batched fast path.  Virtual env: chain c steps the SE with weights theta + sign[c]*eps[worker[c]], `repeat` times on the same action
        (what `same_action_num` does in `step`: rewards summed, next state / done of the last step).
        Discrete action space: actions int32 [chains] (or [chains,n]); continuous: fp32 [chains,A] (or [chains,n,A]).
        states fp32 [chains,S] (or [chains,n,S]), all on the device.  Returns device tensors.
        Reward env over a vector-state real env (or the bare real env: reward type 0): chain c steps its own instance of the real env, up to
        `repeat` times and until it reports done, and shapes the rewards with the reward net theta + sign[c]*eps[worker[c]]; `states` is the
        PopulationState of `reset_population`, advanced in place; actions int32 [chains] / fp32 [chains,A]; gamma is the value
        `set_agent_params` stored.  Returns device tensors (obs, reward, done)."""
        if not self.is_virtual_env():
            real = self._real_env()
            rn = self.env if isinstance(self.env, RewardEnv) else None
            rtype = rn.reward_env_type if rn is not None else 0
            gamma = rn.gamma if rn is not None and rn.gamma is not None else 0.0
            obs, reward, done = engine.rn_step_population(
                real.env_id, self.max_episode_steps(), rtype, rn.desc() if rn is not None else None, rn.info_dim if rn is not None else 0, gamma,
                rn.step_params() if rn is not None else None, rn.step_eps(eps) if rn is not None else None, worker, sign, actions, states.state,
                states.elapsed, repeat=repeat)
            states.obs = obs
            return obs, reward, done
        args = (self.env.descs(), self.env.step_params(), self.env.step_eps(eps), worker, sign, states)
        if not self.has_discrete_action_space():
            return engine.se_step_population_vec(*args, actions, repeat=repeat)
        if repeat == 1:
            return engine.se_step_population(*args, actions)
        one_hot = torch.nn.functional.one_hot(actions.long(), self.get_action_dim()).to(torch.float32)
        return engine.se_step_population_vec(*args, one_hot, repeat=repeat)

    def reset(self):
        """CPU fp32 state of a fresh episode; a virtual env over a discrete observation space hands back the index."""
        first = self.env.reset()
        if torch.is_tensor(first):
            out = first.cpu()
        elif isinstance(first, np.ndarray):
            out = torch.from_numpy(first).float().cpu()
        else:                                          # a gridworld's integer state
            out = torch.tensor([first], device="cpu", dtype=torch.float32)
        discrete_virtual = self.is_virtual_env() and self.has_discrete_state_space()
        return from_one_hot_encoding(out) if discrete_virtual else out

    def get_random_action(self):
        space = self.env.action_space
        if isinstance(space, Discrete):
            return torch.tensor([int(np.random.randint(space.n))], device="cpu", dtype=torch.float32)
        return torch.from_numpy(np.random.uniform(space.low, space.high).astype(np.float32))

    def get_state_dim(self):
        if self.env.observation_space.shape:
            return self.env.observation_space.shape[0]
        return self.env.observation_space.n

    def get_action_dim(self):
        if self.env.action_space.shape:
            return self.env.action_space.shape[0]
        return self.env.action_space.n

    def get_max_action(self):
        return 2 if self.env.env_name == 'Pendulum-v0' else 1

    def get_min_action(self):
        return 0 if self.env.env_name == 'CartPole-v0' else -self.get_max_action()

    def has_discrete_action_space(self):
        return isinstance(self.env.action_space, Discrete)

    def has_discrete_state_space(self):
        return isinstance(self.env.observation_space, Discrete)

    def render(self):
        return None

    def close(self):
        if not self.is_virtual_env():
            return self.env.close()

    def get_solved_reward(self):
        return self.env.solved_reward

    def max_episode_steps(self):
        return self.env._max_episode_steps

    def can_be_solved(self):
        return self.env.solved_reward < 1e9

    def seed(self, seed):
        """Real envs forward the seed; a virtual env has no RNG of its own to seed (its resets come from `reset_env`)."""
        if self.is_virtual_env():
            print("EnvWrapper.seed: a virtual env is not seeded (its reset states come from the real env)")
            return 0
        return self.env.seed(seed)

    def is_virtual_env(self):
        return isinstance(self.env, VirtualEnv)

    def set_agent_params(self, same_action_num, gamma):
        self.same_action_num = same_action_num
        if hasattr(self.env, "set_agent_params"):
            self.env.set_agent_params(gamma=gamma)
