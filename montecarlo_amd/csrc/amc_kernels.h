// amc_kernels.h -- HIP kernels of the many-chain Metropolis engine (gfx950 / CDNA4).
//
// Data layout in HBM: SoA, one f64 per chain
//   x[M_pad]                      chain positions (Particle.x); e is NOT stored: it is
//                                 potential(x) by construction (particle_1d.jl:13-15,33)
//   beta[M_pad]      (optional)   per-chain Particle.beta
//   acc[K][M_pad], tot[K-1][M_pad]  u32 Move.accepted_calls / total_calls (when kept; the last move's total_calls is the
//                                 step count minus the other moves': every chain takes the same number of steps)
//   ptab[PT_ROWS][AMC_MAX_MOVES]  per-move derived parameters (device-computed)
// One lane owns TWO adjacent chains (one global "pair"): 16-byte loads/stores, one
// Box-Muller and one accept-uniform Philox call serve both chains.
// All kernels are HBM-streaming in shape but f64-VALU-bound in practice; no MFMA.
//
// The sources, in include order (each includes its predecessor; hiprtc gets all of them by name, embed_sources.py):
//   amc_model.h        configuration, script-defined hooks, potential / proposal / acceptance, one mc_step! of a chain pair
//   amc_wave_sums.h    device side of the reproducible cross-chain sums (wave totals, lane accumulators, block rows)
//   amc_sweep.h        K1: sweep_kernel, the step log and its fold into the per-chain counters
//   amc_params.h       initial ensemble, parameter / pick tables, the device-resident learning step
//   amc_reduce_pass.h  K2a: the callback reductions as a pass of their own; counter passes
//   amc_pg_tail.h      estimator launch records, GradientData samples, accumulate / update kernels, pending learning steps
//   amc_estimator.h    K3: pg_estimate_kernel (optionally fused with the sweep and the callback sums)
//   amc_aux_kernels.h  histogram / energy / conversion kernels, parity-test hooks
//   amc_exchange.h     replica exchange along a temperature ladder: exchange_kernel, the histogram by rung; the rung and bridge sums and
//                      the frame of every sum by group (slot prologue, block end, finishing merge)
//   amc_anneal.h       population annealing: log-weights, integer weights, the three-launch prefix, the gather, the families
//   amc_anneal_search.h  population annealing: the next beta from a target on the effective-sample fraction (energies, sums, decision)
//   amc_corr.h         time correlation from one time origin: the sums of O, O^2, a O by group, one slot per lag
//   amc_blocks.h       jackknife blocks: the traversal's index arithmetic, the bridge sums and the time correlation per block of ladders
//   amc_ehist.h        the passes over the energy bins: a HIP block's cells (set up, flushed) and the three traversals of the chains
//                      (by group, by jackknife block, by family), each once; the energy histograms per group:
//                      energy_histogram_kernel, energy_histogram_blocks_kernel (a set of rows per jackknife block),
//                      energy_histogram_families_kernel (a row per block of families); an accumulator's words zeroed behind a
//                      respacing, its blocks' sets folded into one
//   amc_emom.h         moments per energy bin: the same cells and traversals with integer sums of x, x^2 and [x > 0] per bin beside
//                      the counts (energy_moments_kernel, energy_moments_blocks_kernel), the deposit rule the host compiles too
//   amc_chainstats.h   convergence per group: running sums per chain (chain_stats_add_kernel) and their sums by group
#pragma once

#include "amc_model.h"
#include "amc_wave_sums.h"
#include "amc_sweep.h"
#include "amc_params.h"
#include "amc_reduce_pass.h"
#include "amc_pg_tail.h"
#include "amc_estimator.h"
#include "amc_aux_kernels.h"
#include "amc_exchange.h"
#include "amc_anneal.h"
#include "amc_anneal_search.h"
#include "amc_corr.h"
#include "amc_blocks.h"
#include "amc_ehist.h"
#include "amc_emom.h"
#include "amc_chainstats.h"
