"""CFR algorithms (reference: src/algorithms/__init__.py -- same exported names)."""
from .vanilla_cfr import CFRTrainer, InfoNode, LearnedCFRPolicy, RandomPolicy
from .mc_cfr import MCCFRTrainer, ScopaLearnedPolicy
from .evaluation import best_response, check_policy_table, cross_play, evaluate_agent_device
from .cfr_variants import schedule
from .team_cfr import TeamCFRTrainer
from .team_mccfr import TeamMCCFRTrainer
from .full_mccfr import FullMCCFRTrainer
from .full_chance import FullChanceMCCFRTrainer, packet_decks, sample_decks

__all__ = ["CFRTrainer", "InfoNode", "LearnedCFRPolicy", "RandomPolicy", "MCCFRTrainer", "ScopaLearnedPolicy", "evaluate_agent_device", "schedule", "cross_play", "best_response",
           "check_policy_table", "solve_mccfr", "TeamCFRTrainer", "TeamMCCFRTrainer", "FullMCCFRTrainer", "FullChanceMCCFRTrainer", "packet_decks", "sample_decks"]
from . import chance
from . import team_chance
from . import full_chance            # full_chance.cross_play, full_chance.evaluate: FullScopa over decks, store against store
from .chance import solve_mccfr
