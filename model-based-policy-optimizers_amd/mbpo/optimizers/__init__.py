"""mbpo.optimizers — same exports as the reference (mbpo/optimizers/__init__.py:1-6) for the hot path."""
from mbpo.optimizers.base_optimizer import BaseOptimizer
from mbpo.optimizers.policy_optimizers.brax_optimizers import BraxOptimizer, BraxOutput, BraxState, PPOOptimizer, SACOptimizer
from mbpo.optimizers.policy_optimizers.bptt_optimizer import BPTTOptimizer, BPTTState
from mbpo.optimizers.policy_optimizers.sac.sac import SAC
from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCEMOptimizer, iCemOptimizerState, iCemParams, iCemTO
from mbpo.optimizers.trajectory_optimizers.policy_prior import PolicyPrior            # (not in the reference: the actor among iCEM's candidates)
from mbpo.optimizers.trajectory_optimizers.terminal_value import TerminalValue      # (not in the reference: a critic at iCEM's horizon)
