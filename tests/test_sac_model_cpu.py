"""CPU: SAC_Policy (policy/SAC_model.py) against the reference's own SAC networks (tests/golden/learn_sac_init.npz,
learn_sac.npz): the reference's state_dict keys load as they are, the seeded initialisation is the reference's, the
sampled action, its log-probability and both critics' q on the recorded state and recorded eps are the recorded ones,
and checkpoints keep the reference's six file names."""
import json
import os

import numpy as np
import torch

from sac_helpers import NETS, golden, load_sd, policy


def _act_state(z):
    obj = torch.tensor(z["act/state_obj"], dtype=torch.float32)
    n = obj.shape[0]
    x2, mask = torch.zeros(1, 5, 5), torch.zeros(1, 5)
    x2[0, :n] = obj
    mask[0, :n] = 1.0
    return torch.tensor(z["act/state_self"], dtype=torch.float32).reshape(1, 7), x2, mask


def test_reference_weights_give_the_recorded_sample_and_q():
    zi, zf = golden()
    pol = policy("cpu", seed=3)   # another seed: every weight comes from the fixture
    load_sd(pol, zi, "init/")
    s = _act_state(zi)
    with torch.no_grad():
        a, logp = pol.actor(s, eps=torch.tensor(zi["act/eps"]))
        q1, q2 = pol.critic_1(s, a), pol.critic_2(s, a)
    assert a.shape == (1, 2) and logp.shape == (1, 1) and q1.shape == (1, 1)
    # f32 results of the same layers; 1e-6 leaves room for another CPU's GEMM summation order
    np.testing.assert_allclose(a.numpy(), zi["act/action"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(logp.numpy(), zi["act/logp"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(q1.numpy(), zi["act/q1"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(q2.numpy(), zi["act/q2"], rtol=0, atol=1e-6)
    assert not np.allclose(zi["act/q1"], zi["act/q2"])   # the twins differ (seeds 101, 102)
    load_sd(pol, zf, "after1/")   # the trained weights load strictly too


def test_eps_none_draws_as_the_reference_does():
    """forward(x) without eps is Normal.rsample: the torch generator's next (1, 2) standard normals."""
    zi, _ = golden()
    pol = policy("cpu")
    s = _act_state(zi)
    torch.manual_seed(5)
    eps = torch.randn(1, 2)
    torch.manual_seed(5)
    with torch.no_grad():
        a, logp = pol.actor(s)
        a2, logp2 = pol.actor(s, eps=eps)
    np.testing.assert_allclose(a.numpy(), a2.numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(logp.numpy(), logp2.numpy(), rtol=0, atol=1e-5)


def test_seeded_initialisation_is_the_reference_s():
    """Same constructor arguments and seeds (actor: seed, critics: seed + 1, seed + 2) -> the reference's weights."""
    zi, _ = golden()
    pol = policy("cpu")
    for kind in NETS:
        sd = getattr(pol, kind).state_dict()
        keys = [k[len(f"init/{kind}/"):] for k in zi.files if k.startswith(f"init/{kind}/")]
        assert list(sd) == keys
        for k, v in sd.items():
            np.testing.assert_array_equal(v.numpy(), zi[f"init/{kind}/{k}"], err_msg=f"{kind}/{k}")
    assert bool(zi["target/equals_init"]) and float(zi["alpha"]) == 0.078


def test_save_load_round_trip(tmp_path):
    from distributional_rl_decision_and_control_amd.policy.SAC_model import Actor, Critic, SAC_Policy
    _, zf = golden()
    pol = policy("cpu", seed=9)
    load_sd(pol, zf, "after1/")
    pol.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["actor_constructor_params.json", "actor_network_params.pth",
                                            "critic_1_constructor_params.json", "critic_1_params.pth",
                                            "critic_2_constructor_params.json", "critic_2_params.pth"]
    with open(tmp_path / "actor_constructor_params.json") as f:
        assert set(json.load(f)) == {"self_dimension", "object_dimension", "max_object_num", "self_feature_dimension",
                                     "object_feature_dimension", "concat_feature_dimension", "hidden_dimension",
                                     "value_ranges_of_action", "seed"}
    with open(tmp_path / "critic_2_constructor_params.json") as f:
        assert set(json.load(f)) == {"self_dimension", "object_dimension", "max_object_num", "self_feature_dimension",
                                     "object_feature_dimension", "concat_feature_dimension", "hidden_dimension",
                                     "action_dimension", "seed"}
    back = SAC_Policy.load(str(tmp_path))
    assert isinstance(back.actor, Actor) and isinstance(back.critic_1, Critic) and isinstance(back.critic_2, Critic)
    for kind in NETS:
        a, b = getattr(pol, kind).state_dict(), getattr(back, kind).state_dict()
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (kind, k)
