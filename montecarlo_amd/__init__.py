"""montecarlo_amd: MI355X-native many-chain Metropolis engine behind Arianna.jl's plugin API.

The compute path is libamc.so (hand-written HIP for gfx950, C ABI in include/amc.h).  This
package is the host-side mirror of the reference's interface for that one path -- Move / pool /
Simulation / run -- so a user of TheDisorderedOrganization/MonteCarlo's particle_1d examples finds
the same names.  There is no CPU implementation here: without the built extension and a GPU,
constructing ``Metropolis`` raises.
"""
from ._capi import AmcError, HipEngine, SplitEngine, device_count
from .metropolis import Metropolis, callback_acceptance, callback_energy, callback_moments
from .policy_guided import (ANPG, BLANPG, BLAPG, BLPG, NPG, VPG, GradientData, PolicyGradientEstimator,
                            PolicyGradientUpdate, Static, average, initialise_gradient_data, learning_step,
                            log_proposal_density, withgrad_log_proposal_density)
from . import sharding
from .sharding import allreduce_sum, init_store_group, shard_range
from .simulation import (AriannaAlgorithm, PrintTimeSteps, Simulation, StoreCallbacks, StoreParameters,
                         build_schedule, julia_repr, run)
from .exchange import (ReplicaExchange, callback_exchange_acceptance, callback_rung_acceptance, callback_flow_fraction, callback_round_trips, callback_rung_energy,
                       callback_rung_moments, rung_energy, RespaceLadder, callback_ladder, TuneRungSigma, callback_rung_sigma,
                       callback_rung_window_acceptance, callback_log_z, callback_heat_capacity, callback_log_z_error,
                       callback_heat_capacity_error)
from .correlation import Autocorrelation, callback_rho, callback_tau_int, callback_tau_int_error, rho_from_records, tau_from_rho
from .convergence import Convergence, callback_rhat, rhat_from_records, tau_batch_from_records, variances_from_records
from .energy_histogram import (EnergyHistogram, callback_reweight_error, callback_reweight_moments,
                               callback_reweight_moments_error)
from . import reweighting
from .annealing import ANNEAL_SEARCH_STATUS, PopulationAnnealing, callback_anneal_beta, callback_anneal_log_z, callback_anneal_log_z_error, callback_rho_t
from .storage import StoreHistogram, StoreSnapshots, checkpoint, restore
from .trajectories import DAT, TXT, StoreBackups, StoreLastFrames, StoreTrajectories
from .system import Action, AriannaSystem, Policy
from .system import CustomPotential, Displacement, Move, ParticleChains, ScaledGaussian, ScriptAction, ScriptPolicy, StandardGaussian, potential

__all__ = [
    "AmcError", "HipEngine", "SplitEngine", "device_count",
    "Metropolis", "callback_acceptance", "callback_energy", "callback_moments",
    "ANPG", "BLANPG", "BLAPG", "BLPG", "NPG", "VPG", "Static", "GradientData", "PolicyGradientEstimator",
    "PolicyGradientUpdate", "average", "initialise_gradient_data", "learning_step",
    "log_proposal_density", "withgrad_log_proposal_density",
    "allreduce_sum", "init_store_group", "shard_range", "sharding",
    "AriannaAlgorithm", "PrintTimeSteps", "Simulation", "StoreCallbacks", "StoreParameters",
    "build_schedule", "julia_repr", "run",
    "StoreHistogram", "StoreSnapshots", "checkpoint", "restore",
    "ReplicaExchange", "callback_exchange_acceptance", "callback_rung_acceptance", "callback_flow_fraction", "callback_round_trips", "callback_rung_energy",
    "callback_rung_moments", "rung_energy", "RespaceLadder", "callback_ladder", "TuneRungSigma", "callback_rung_sigma",
    "callback_rung_window_acceptance", "callback_log_z", "callback_heat_capacity", "callback_log_z_error", "callback_heat_capacity_error",
    "Autocorrelation", "callback_rho", "callback_tau_int", "callback_tau_int_error", "rho_from_records", "tau_from_rho",
    "Convergence", "callback_rhat", "rhat_from_records", "tau_batch_from_records", "variances_from_records",
    "EnergyHistogram", "callback_reweight_error", "callback_reweight_moments", "callback_reweight_moments_error", "reweighting",
    "ANNEAL_SEARCH_STATUS", "PopulationAnnealing", "callback_anneal_beta", "callback_anneal_log_z", "callback_anneal_log_z_error", "callback_rho_t",
    "DAT", "TXT", "StoreBackups", "StoreLastFrames", "StoreTrajectories",
    "Action", "AriannaSystem", "Policy", "CustomPotential", "Displacement", "Move", "ParticleChains", "ScaledGaussian", "ScriptAction", "ScriptPolicy", "StandardGaussian", "potential",
]
