"""experiments/transfer_cartpole.py on the GPU: the replay of the reference scripts' own runs (fixtures g18) equals the oracle bit for bit,
train_test_agents_models equals the per-model calls agent for agent, and the episodes per launch do not change a bit of what is returned."""
import copy
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_transfer_cartpole_reference import G18, TAPES, g18_launch_config, g18_oracle_chain  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = "CartPole-v0"
SMALL = dict(train_episodes=5, init_episodes=1, rb_size=1000000)


def _reward_env_and_real_env(cfg, seed):
    from learning_environments_amd.envs.env_factory import EnvFactory
    torch.manual_seed(seed)
    fac = EnvFactory(copy.deepcopy(cfg))
    return fac.generate_reward_env(), fac.generate_real_env()


@pytest.fixture(scope="module")
def setup():
    from learning_environments_amd import engine
    from learning_environments_amd.experiments import transfer_cartpole as tc
    engine.require_device()
    base = tc.base_config()
    base["envs"][ENV].update(max_steps=25, hidden_size=32)
    envs = [_reward_env_and_real_env(base, s) for s in (1, 2, 3)]
    return tc, base, envs


@pytest.mark.parametrize("name", G18)
def test_fixture_replay_equals_the_oracle_bit_for_bit(golden, name):
    """A run of the reference script's own train_test_agents (fixtures g18) replayed through the module on the GPU -- recorded hyper-parameters,
    fresh agents, ICMs and draws, two episodes per launch -- returns the oracle's lists bit for bit, and the script's within 1e-5 / exactly."""
    from oracle import oracle as orc
    from learning_environments_amd import engine
    from learning_environments_amd.experiments import transfer_cartpole as tc
    engine.require_device()
    g = golden(name)
    mode, script, _, cfgd = g18_launch_config(g)
    n_ag = int(g["agents"])
    cut = json.loads(str(g["cut_json"]))
    config = json.loads(str(g["config_before_json"]))
    reward_env, real_env = _reward_env_and_real_env(config, 0)
    hps = [json.loads(str(g["a%d_hp_json" % i])) for i in range(n_ag)]
    replay = dict(theta=g["theta"], agent_init=[g["a%d_agent_init" % i] for i in range(n_ag)], icm=cut["icm"],
                  icm_init=[g["a%d_icm_init" % i] for i in range(n_ag)] if mode == "-1" else None,
                  tapes=[{k: g["a%d_tape_%s" % (i, k)] for k in TAPES} for i in range(n_ag)])
    env = real_env if mode in ("0", "-1") else reward_env
    (rewards, lengths), launch = tc.train_test_agents(mode, env, real_env, config, script=script, agents_num=n_ag, settings=cut["agent"], hps=hps,
                                                      replay=replay, episodes_per_launch=2, details=True)
    assert config["agents"][tc.SECTION[script]]["train_episodes"] == cut["agent"]["train_episodes"] and config["agents"]["icm"]["feature_dim"] == 8
    assert launch["cfg"].q_hidden == max(h["hidden_size"] for h in hps) and launch["cfg"].agent_kind == int(script == "algo")
    for i in range(n_ag):
        p = "a%d_" % i
        _, o, _ = g18_oracle_chain(orc, g, i, cfgd, mode)
        assert o["rc"] == 0
        assert rewards[i] == o["episode_test_mean"].tolist() and lengths[i] == o["episode_len"].tolist(), (name, i)
        assert np.abs(np.array(rewards[i]) - g[p + "rewards"]).max() <= 1e-5 and lengths[i] == g[p + "episode_lengths"].tolist()


@pytest.mark.parametrize("script,mode", [("vary_hp", "2"), ("algo", "-1")])
def test_models_launch_equals_the_per_model_calls(setup, script, mode):
    tc, base, envs = setup
    both, launch = tc.train_test_agents_models(mode, [e[0] for e in envs], envs[0][1], copy.deepcopy(base), script=script, agents_num=2, seed=9,
                                               settings=SMALL, episodes_per_launch=2, details=True)
    assert len(both) == 3 and launch["inner"].chains == 6
    if script == "vary_hp":                                  # every agent draws its own shapes from its key (model index, agent index)
        assert len({(h["hidden_size"], h["batch_size"]) for h in launch["hps"]}) == 6
    else:
        assert all(h == dict(lr=0.00025, batch_size=32, hidden_size=64, hidden_layer=1) for h in launch["hps"]) and launch["cfg"].feature_dim == 128
    for mi in range(3):
        single = tc.train_test_agents(mode, envs[mi][0], envs[0][1], copy.deepcopy(base), script=script, agents_num=2, seed=9, model_index=mi,
                                      settings=SMALL, episodes_per_launch=None)
        assert both[mi] == single, (script, mi)
        assert all(len(r) == 5 and np.isfinite(r).all() for r in single[0])
    if mode == "2":
        assert both[0] != both[1]
        with pytest.raises(ValueError, match="reward_env_type"):
            tc.train_test_agents("5", envs[0][0], envs[0][1], copy.deepcopy(base), script=script, agents_num=2, settings=SMALL)


@pytest.mark.parametrize("script,mode", [("vary_hp", "-1"), ("algo", "2")])
def test_episodes_per_launch_does_not_change_what_is_returned(setup, script, mode):
    tc, base, envs = setup
    got, calls = {}, []
    for epl in (None, 2):
        got[epl] = tc.train_test_agents(mode, envs[0][0], envs[0][1], copy.deepcopy(base), script=script, agents_num=3, seed=5, settings=SMALL,
                                        episodes_per_launch=epl, on_segment=lambda done, fin: calls.append((epl, done, fin)))
    assert got[None] == got[2]
    assert calls == [(2, 2, 0), (2, 4, 0), (2, 5, 3)]        # once per segment, with the cumulative state
