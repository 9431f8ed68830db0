"""SAC actor / twin critics (rfarl/rfarl/policy/SAC_model.py:19-356): the second continuous-action baseline AC-IQN
is compared against. Same constructor arguments, layer names (state_dict keys), seeded initialisation order (actor
`seed`, critics `seed + 1` and `seed + 2`) and checkpoint files (actor_network_params.pth +
actor_constructor_params.json, critic_{1,2}_params.pth + critic_{1,2}_constructor_params.json) as the reference, so
checkpoints move between the two.

The Critic is DDPG_model.Critic line for line and is that class under SAC's file names. The Actor is the AC-IQN / DDPG
trunk under two 128 -> 2 heads (mean and log standard deviation) with a reparameterised sample squashed by
(2/pi) atan. The one addition: forward() accepts a pre-drawn standard normal `eps` (parity tests, the kernels'
restatement); eps=None draws as the reference does (Normal.rsample)."""
import copy
import json
import math
import os

import torch
import torch.nn as nn
from torch.distributions import Normal
from torch.nn.functional import relu

from .AC_IQN_model import _Saveable, encode_observation, encoder
from .DDPG_model import Critic as _DDPGCritic


class SAC_Policy:
    def __init__(self, self_dimension, object_dimension, max_object_num, self_feature_dimension,
                 object_feature_dimension, concat_feature_dimension, hidden_dimension, value_ranges_of_action,
                 device="cpu", seed=0, min_log_std=-20, max_log_std=2):
        self.actor = Actor(self_dimension, object_dimension, max_object_num, self_feature_dimension,
                           object_feature_dimension, concat_feature_dimension, hidden_dimension,
                           value_ranges_of_action, device, seed, min_log_std, max_log_std).to(device)
        self.critic_1 = Critic(self_dimension, object_dimension, max_object_num, self_feature_dimension,
                               object_feature_dimension, concat_feature_dimension, hidden_dimension,
                               len(value_ranges_of_action), device, seed + 1).to(device)
        self.critic_2 = Critic(self_dimension, object_dimension, max_object_num, self_feature_dimension,
                               object_feature_dimension, concat_feature_dimension, hidden_dimension,
                               len(value_ranges_of_action), device, seed + 2).to(device)

    def save(self, directory):
        self.actor.save(directory)
        self.critic_1.save(1, directory)
        self.critic_2.save(2, directory)

    @classmethod
    def load(cls, directory, device="cpu"):
        actor = Actor.load(directory, device)
        critic_1 = Critic.load(1, directory, device)
        critic_2 = Critic.load(2, directory, device)
        policy = cls(actor.self_dimension, actor.object_dimension, actor.max_object_num,
                     actor.self_feature_dimension, actor.object_feature_dimension, actor.concat_feature_dimension,
                     actor.hidden_dimension, actor.value_ranges_of_action, device=device)
        policy.actor = actor
        policy.critic_1 = critic_1
        policy.critic_2 = critic_2
        return policy


class Actor(_Saveable, nn.Module):
    _prefix = "actor_"

    def __init__(self, self_dimension, object_dimension, max_object_num, self_feature_dimension,
                 object_feature_dimension, concat_feature_dimension, hidden_dimension, value_ranges_of_action,
                 device="cpu", seed=0, min_log_std=-20, max_log_std=2):
        super().__init__()
        self.self_dimension = self_dimension
        self.object_dimension = object_dimension
        self.max_object_num = max_object_num
        self.self_feature_dimension = self_feature_dimension
        self.object_feature_dimension = object_feature_dimension
        self.concat_feature_dimension = concat_feature_dimension
        self.hidden_dimension = hidden_dimension
        self.value_ranges_of_action = copy.deepcopy(value_ranges_of_action)
        self.action_dimension = len(self.value_ranges_of_action)
        self.device = device
        self.seed_id = seed
        self.seed = torch.manual_seed(seed)  # SAC_model.py:129
        self.register_buffer("atan_scale", torch.tensor(2.0 / torch.pi), persistent=False)  # :131
        self.register_buffer("min_val", torch.tensor(1e-6).float(), persistent=False)  # :132
        self.min_log_std = min_log_std
        self.max_log_std = max_log_std
        self.self_encoder = encoder(self_dimension, self_feature_dimension)
        self.object_encoder = encoder(object_dimension, object_feature_dimension)
        self.hidden_layer = nn.Linear(self.concat_feature_dimension, hidden_dimension)
        self.hidden_layer_2 = nn.Linear(hidden_dimension, hidden_dimension)
        self.output_layer_mu = nn.Linear(hidden_dimension, self.action_dimension)
        self.output_layer_log_std = nn.Linear(hidden_dimension, self.action_dimension)

    def observation_processor(self, x):
        assert len(x) == 3, "The number of elements in state must be 3!"
        return encode_observation(self.self_encoder, self.object_encoder, x, self.max_object_num,
                                  self.object_dimension, self.object_feature_dimension)

    def head(self, x):
        """(mu, log_std before the clamp) of SAC_model.py:178-184."""
        features = self.observation_processor(x)
        features = relu(self.hidden_layer(features))
        features = relu(self.hidden_layer_2(features))
        return self.output_layer_mu(features), self.output_layer_log_std(features)

    def forward(self, x, eps=None):  # SAC_model.py:175-187
        mu, log_std = self.head(x)
        log_std = torch.clamp(log_std, self.min_log_std, self.max_log_std)
        return self.compute_action(mu, log_std, eps)

    def compute_action(self, mu, log_std, eps=None):  # SAC_model.py:189-199
        sigma = torch.exp(log_std)
        if eps is None:
            dist = Normal(mu, sigma)
            z = dist.rsample()
            log_prob = dist.log_prob(z)
        else:   # rsample is mu + sigma * eps; log_prob(z) with (z - mu) / sigma = eps
            z = mu + sigma * eps
            log_prob = -(eps ** 2) / 2 - log_std - math.log(math.sqrt(2 * math.pi))
        actions = self.atan_scale * torch.atan(z)  # map to (-1, 1)
        log_prob = log_prob - torch.log(1 - actions.pow(2) + self.min_val)
        return actions, log_prob.sum(dim=-1, keepdim=True)

    def get_constructor_parameters(self):
        return dict(self_dimension=self.self_dimension, object_dimension=self.object_dimension,
                    max_object_num=self.max_object_num, self_feature_dimension=self.self_feature_dimension,
                    object_feature_dimension=self.object_feature_dimension,
                    concat_feature_dimension=self.concat_feature_dimension, hidden_dimension=self.hidden_dimension,
                    value_ranges_of_action=self.value_ranges_of_action, seed=self.seed_id)


class Critic(_DDPGCritic):
    """SAC_model.py:238-356: DDPG's critic; the checkpoint files carry the twin's number."""

    def save(self, id, directory):
        torch.save(self.state_dict(), os.path.join(directory, f"critic_{id}_params.pth"))
        with open(os.path.join(directory, f"critic_{id}_constructor_params.json"), mode="w") as f:
            json.dump(self.get_constructor_parameters(), f)

    @classmethod
    def load(cls, id, directory, device="cpu"):
        params = torch.load(os.path.join(directory, f"critic_{id}_params.pth"), map_location=device,
                            weights_only=True)
        with open(os.path.join(directory, f"critic_{id}_constructor_params.json"), mode="r") as f:
            ctor = json.load(f)
            ctor["device"] = device
        model = cls(**ctor)
        model.load_state_dict(params)
        model.to(device)
        return model
