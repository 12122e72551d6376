"""CPU restatement (torch) of SB3's DQN `CnnPolicy` on top of `tests/sqil_ref.py`: `DQNPolicy` with
`features_extractor_class=NatureCNN` (`oracle.sb3_restated.NatureCNN`) and SB3's default `net_arch=[]` behind it.

Its Q-network casts the preprocessed frames (`x / 255`, float32 as [SB3 preprocess_obs] leaves them) to the parameters'
dtype BEFORE the extractor: `sqil_ref.QNetwork.forward` casts behind the extractor, which is right for the flatten
extractor and breaks the float64 switch on a convolution (float32 input, float64 weights).

It is passed to the reference's `SQIL` as a class (`policy=CnnPolicy`), so no alias table is edited.
"""
from __future__ import annotations

import torch as th
from torch import nn

from oracle import sb3_restated as sb
from tests import sqil_ref


class CnnQNetwork(sqil_ref.QNetwork):
    def forward(self, obs: th.Tensor) -> th.Tensor:
        x = sb.preprocess_obs(obs, self.observation_space, self.normalize_images)
        return self.q_net(self.features_extractor(x.to(self.q_net[0].weight.dtype)))


class CnnPolicy(sqil_ref.DQNPolicy):
    def __init__(self, observation_space, action_space, lr_schedule, net_arch=None, activation_fn=nn.ReLU,
                 features_extractor_class=sb.NatureCNN, features_extractor_kwargs=None, normalize_images: bool = True,
                 optimizer_class=th.optim.Adam, optimizer_kwargs=None):
        super().__init__(observation_space, action_space, lr_schedule, [] if net_arch is None else net_arch, activation_fn,
                         features_extractor_class, features_extractor_kwargs, normalize_images, optimizer_class,
                         optimizer_kwargs)

    def make_q_net(self) -> CnnQNetwork:
        fe = self.make_features_extractor()
        return CnnQNetwork(self.observation_space, self.action_space, fe, fe.features_dim, self.net_arch,
                           self.activation_fn, self.normalize_images)

    def obs_to_tensor(self, observation):
        # (frames stay uint8 up to `preprocess_obs`; `sqil_ref.DQNPolicy.obs_to_tensor` would cast them first)
        return sb.BasePolicy.obs_to_tensor(self, observation)
