"""DDPG actor / critic (rfarl/rfarl/policy/DDPG_model.py:16-318): the continuous-action baseline AC-IQN is
compared against. Same constructor arguments, layer names (state_dict keys), seeded initialisation order and
checkpoint files (actor_network_params.pth + actor_constructor_params.json, critic_...) as the reference, so
checkpoints move between the two.

The Actor is the AC-IQN Actor layer for layer (AC_IQN_model.Actor: both encoders, 256 -> 128 -> 128 -> 2,
(2/pi) atan) and is that class under DDPG's name. The Critic is the AC-IQN critic without the cosine embedding
and with one scalar per sample."""
import torch
import torch.nn as nn
from torch.nn.functional import relu

from .AC_IQN_model import Actor as _ACIQNActor
from .AC_IQN_model import _Saveable, encode_observation, encoder


class DDPG_Policy:
    def __init__(self, self_dimension, object_dimension, max_object_num, self_feature_dimension,
                 object_feature_dimension, concat_feature_dimension, hidden_dimension, value_ranges_of_action,
                 device="cpu", seed=0):
        self.actor = Actor(self_dimension, object_dimension, max_object_num, self_feature_dimension,
                           object_feature_dimension, concat_feature_dimension, hidden_dimension,
                           value_ranges_of_action, device, seed).to(device)
        self.critic = Critic(self_dimension, object_dimension, max_object_num, self_feature_dimension,
                             object_feature_dimension, concat_feature_dimension, hidden_dimension,
                             len(value_ranges_of_action), device, seed + 1).to(device)

    def save(self, directory):
        self.actor.save(directory)
        self.critic.save(directory)

    @classmethod
    def load(cls, directory, device="cpu"):
        actor = Actor.load(directory, device)
        critic = Critic.load(directory, device)
        policy = cls(actor.self_dimension, actor.object_dimension, actor.max_object_num,
                     actor.self_feature_dimension, actor.object_feature_dimension, actor.concat_feature_dimension,
                     actor.hidden_dimension, actor.value_ranges_of_action, device=device)
        policy.actor = actor
        policy.critic = critic
        return policy


class Actor(_ACIQNActor):
    """DDPG_model.py:81-197: the same layers, forward and checkpoint files as the AC-IQN Actor."""


class Critic(_Saveable, nn.Module):
    _prefix = "critic_"

    def __init__(self, self_dimension, object_dimension, max_object_num, self_feature_dimension,
                 object_feature_dimension, concat_feature_dimension, hidden_dimension, action_dimension,
                 device="cpu", seed=0):
        super().__init__()
        self.self_dimension = self_dimension
        self.object_dimension = object_dimension
        self.max_object_num = max_object_num
        self.self_feature_dimension = self_feature_dimension
        self.object_feature_dimension = object_feature_dimension
        self.concat_feature_dimension = concat_feature_dimension
        self.hidden_dimension = hidden_dimension
        self.action_dimension = action_dimension
        self.device = device
        self.seed_id = seed
        self.seed = torch.manual_seed(seed)  # DDPG_model.py:225
        self.self_encoder = encoder(self_dimension, self_feature_dimension)
        self.object_encoder = encoder(object_dimension, object_feature_dimension)
        self.action_encoder = encoder(self.action_dimension, hidden_dimension)
        self.hidden_layer = nn.Linear(self.concat_feature_dimension, hidden_dimension)
        self.hidden_layer_2 = nn.Linear(hidden_dimension, hidden_dimension)
        self.output_layer = nn.Linear(hidden_dimension, 1)

    def observation_processor(self, x):
        assert len(x) == 3, "The number of elements in state must be 3!"
        return encode_observation(self.self_encoder, self.object_encoder, x, self.max_object_num,
                                  self.object_dimension, self.object_feature_dimension)

    def forward(self, x, actions):  # DDPG_model.py:267-282
        features = relu(self.hidden_layer(self.observation_processor(x)))
        features = self.action_encoder(actions) * features
        features = relu(self.hidden_layer_2(features))
        return self.output_layer(features)

    def get_constructor_parameters(self):
        return dict(self_dimension=self.self_dimension, object_dimension=self.object_dimension,
                    max_object_num=self.max_object_num, self_feature_dimension=self.self_feature_dimension,
                    object_feature_dimension=self.object_feature_dimension,
                    concat_feature_dimension=self.concat_feature_dimension, hidden_dimension=self.hidden_dimension,
                    action_dimension=self.action_dimension, seed=self.seed_id)
