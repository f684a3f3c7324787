from .deep_cfr import AdvantageNetwork, DeepCFR, DeviceMemory, RandomPolicy, StrategyBuffer
from .chance_deep_cfr import ChanceDeepCFR
from .team_chance_deep_cfr import TeamChanceDeepCFR
from .full_chance_deep_cfr import FullChanceDeepCFR
from .nets import FlexibleNet, MLPBlock, masked_softmax, positive_regret_policy

__all__ = ["DeepCFR", "ChanceDeepCFR", "TeamChanceDeepCFR", "FullChanceDeepCFR", "AdvantageNetwork", "StrategyBuffer", "DeviceMemory", "RandomPolicy", "FlexibleNet", "MLPBlock",
           "positive_regret_policy", "masked_softmax"]
