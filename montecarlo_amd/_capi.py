"""ctypes binding of libamc.so (include/amc.h) -- the only way this package computes.

There is no CPU path: if the shared library is missing, or no gfx950 device is
usable, construction raises.  The library is built in-tree by
``__graft_entry__.build()`` / ``make -C montecarlo_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libamc.so")

AMC_MAX_MOVES = 64
AMC_MAX_LEARN = 8
AMC_RED_HEADER = 4
AMC_GD_STRIDE = 5
AMC_XSUM_WORDS = 12      # doubles per record of a reproducible sum (include/amc.h)
AMC_ANNEAL_RECORD_WORDS = 8     # 64-bit words per record of an annealing step
AMC_ANNEAL_MAX_RECORDS = 4096
AMC_ANNEAL_WEIGHT_BITS = 30
AMC_ANNEAL_SEARCH_CANDIDATES = 8    # candidates per round of amc_anneal_next_beta
AMC_ANNEAL_SEARCH_WORDS = 8         # 64-bit words of its diag
AMC_ANNEAL_SEARCH_MAX_ROUNDS = 16
# status of a search (diag[0])
(AMC_ANNEAL_SEARCH_OK, AMC_ANNEAL_SEARCH_LIMIT, AMC_ANNEAL_SEARCH_BELOW_RESOLUTION, AMC_ANNEAL_SEARCH_STALLED, AMC_ANNEAL_SEARCH_ALL_NAN,
 AMC_ANNEAL_SEARCH_INF, AMC_ANNEAL_SEARCH_NO_WEIGHT) = range(7)
AMC_REDUCE_E, AMC_REDUCE_X, AMC_REDUCE_XX, AMC_REDUCE_ALL = 1, 2, 4, 7      # the sums over x a reduction forms (include/amc.h)
# the columns of the bridge sums (include/amc.h); record order E, EE, WF, WB, MF, MB
AMC_BRIDGE_E, AMC_BRIDGE_EE, AMC_BRIDGE_WF, AMC_BRIDGE_WB, AMC_BRIDGE_MF, AMC_BRIDGE_MB, AMC_BRIDGE_ALL = 1, 2, 4, 8, 16, 32, 63
# time correlation (include/amc.h): the observables, the slots of one mark, the columns of a record in their order
AMC_CORR_E, AMC_CORR_X = 1, 2
AMC_CORR_MAX_LAGS = 256
AMC_MAX_JK_BLOCKS = 64          # blocks of a jackknife partition (amc_set_blocks)
AMC_EMOM_X, AMC_EMOM_XX, AMC_EMOM_POS, AMC_EMOM_ALL = 1, 2, 4, 7      # columns of amc_energy_moments_accumulate, in mask-bit order
AMC_EHIST_MAX_BINS = 8192       # bins of any histogram entry (amc_histogram, amc_energy_histogram_accumulate)
AMC_CORR_O, AMC_CORR_OO, AMC_CORR_AO, AMC_CORR_COLS = 0, 1, 2, 3
CORR_OBSERVABLES = {"energy": AMC_CORR_E, "x": AMC_CORR_X}
# convergence per group (include/amc.h): the parts of the window, the columns of a fetch in their order
AMC_CHAIN_STATS_PARTS, AMC_CHAIN_STATS_COLS = 2, 7
(AMC_CHAIN_STATS_S0, AMC_CHAIN_STATS_S0S0, AMC_CHAIN_STATS_Q0, AMC_CHAIN_STATS_S1, AMC_CHAIN_STATS_S1S1, AMC_CHAIN_STATS_Q1,
 AMC_CHAIN_STATS_S0S1) = range(7)
AMC_RESPACE_ACCEPTANCE, AMC_RESPACE_FLOW = 1, 2      # the rules of amc_respace_ladder (include/amc.h)
RESPACE_RULES = {"acceptance": AMC_RESPACE_ACCEPTANCE, "flow": AMC_RESPACE_FLOW}

POTENTIALS = {"harmonic": 0, "double_well": 1}
AMC_POTENTIAL_CUSTOM = 2


class AmcError(RuntimeError):
    """Non-zero amc_status from the C ABI (the Julia binding calls error(...) likewise)."""


class AmcConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("n_chains", C.c_int64),
        ("chain_offset", C.c_int64),
        ("n_chains_global", C.c_int64),
        ("potential", C.c_int32),
        ("n_moves", C.c_int32),
        ("beta", C.c_double),
        ("sigma", C.POINTER(C.c_double)),
        ("weight", C.POINTER(C.c_double)),
        ("seed", C.c_uint64),
        ("sweepstep", C.c_int32),
        ("per_chain_counters", C.c_int32),
        ("stream", C.c_void_p),
        ("state_dtype", C.c_int32),
        ("param_dtype", C.c_int32),
    ]


# amc_state_dtype: Particle{T} (particle_1d.jl:9).  "f64" is the parity type; "f32" keeps x, beta, e, delta in Float32.
STATE_DTYPES = {"f64": 0, "f32": 1, "float64": 0, "float32": 1}


_lib = None
SIGNATURES: dict = {}          # name -> (restype, argtypes) of every bound entry point (filled by load(); tests walk it)


def load() -> C.CDLL:
    """Load libamc.so; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmcError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C montecarlo_amd/csrc). "
            "montecarlo_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    H = C.c_void_p
    dp = C.POINTER(C.c_double)
    i64p = C.POINTER(C.c_int64)
    u64p = C.POINTER(C.c_uint64)
    ip = C.POINTER(C.c_int)
    sp, spp = C.c_char_p, C.POINTER(C.c_char_p)          # const char *, const char *const *
    cfgp, Hp = C.POINTER(AmcConfig), C.POINTER(H)
    sig = {
        "amc_last_error": (sp, []),
        "amc_version": (C.c_int, []),
        "amc_device_count": (C.c_int, [ip]),
        "amc_create": (C.c_int, [cfgp, Hp]),
        "amc_create_custom": (C.c_int, [cfgp, sp, Hp]),
        "amc_create_model": (C.c_int, [cfgp, sp, sp, Hp]),
        "amc_create_policy_model": (C.c_int, [cfgp, sp, sp, sp, Hp]),
        "amc_create_proposal_model": (C.c_int, [cfgp, sp, sp, sp, sp, sp, Hp]),
        "amc_create_action_model": (C.c_int, [cfgp, sp, sp, sp, sp, sp, sp, sp, Hp]),
        "amc_create_vector_policy_model": (C.c_int, [cfgp, C.c_int, sp, sp, sp, sp, spp, sp, sp, Hp]),
        "amc_n_params": (C.c_int, [H, ip, ip]),
        "amc_create_mixed_model": (C.c_int, [cfgp, C.c_int, ip, sp, sp, spp, spp, spp, spp, spp, Hp]),
        "amc_potential_check": (C.c_int, [sp, sp, C.c_int]),
        "amc_destroy": (C.c_int, [H]),
        "amc_upload_state": (C.c_int, [H, dp, dp]),
        "amc_init_uniform": (C.c_int, [H, C.c_double, C.c_double]),
        "amc_download_state": (C.c_int, [H, dp, dp]),
        "amc_download_counters": (C.c_int, [H, i64p, i64p]),
        "amc_counter_totals": (C.c_int, [H, i64p, i64p]),
        "amc_upload_counters": (C.c_int, [H, i64p, i64p]),
        "amc_set_counter_totals": (C.c_int, [H, i64p, C.c_uint64]),
        "amc_histogram": (C.c_int, [H, C.c_double, C.c_double, C.c_int, u64p]),
        "amc_histogram_accumulate": (C.c_int, [H, C.c_double, C.c_double, C.c_int]),
        "amc_histogram_fetch": (C.c_int, [H, u64p, C.c_int, C.c_int]),
        "amc_download_strided": (C.c_int, [H, C.c_int64, C.c_int64, C.c_int64, dp]),
        "amc_get_estimator_step": (C.c_int, [H, u64p]),
        "amc_set_estimator_step": (C.c_int, [H, C.c_uint64]),
        "amc_sweep": (C.c_int, [H, C.c_int64]),
        "amc_sweep_launches": (C.c_int, [H, C.c_int64]),
        "amc_get_step": (C.c_int, [H, u64p]),
        "amc_set_step": (C.c_int, [H, C.c_uint64]),
        "amc_reduce": (C.c_int, [H, dp]),
        "amc_reduce_begin": (C.c_int, [H]),
        "amc_sweep_reduce_begin": (C.c_int, [H, C.c_int64]),
        "amc_reduce_end": (C.c_int, [H, dp]),
        "amc_reduce_end_exact": (C.c_int, [H, dp, u64p]),
        "amc_xsum_merge": (C.c_int, [dp, dp, C.c_int]),
        "amc_xsum_round": (C.c_int, [dp, C.c_int, dp]),
        "amc_pg_estimate_exact": (C.c_int, [H, C.c_int, ip, C.c_int, dp]),
        "amc_pg_route": (C.c_int, [H, C.c_int, C.c_int, C.c_int, sp, C.c_int]),
        "amc_model_check": (C.c_int, [C.c_int, C.c_int, sp, sp, spp, spp, spp, spp, spp, sp, C.c_int]),
        "amc_allreduce_xsum": (C.c_int, [H, dp, C.c_int]),
        "amc_comm_library_forced": (C.c_int, [ip]),
        "amc_set_parameters": (C.c_int, [H, C.c_int, dp, C.c_int]),
        "amc_get_parameters": (C.c_int, [H, C.c_int, dp, C.c_int]),
        "amc_parameters_begin": (C.c_int, [H]),
        "amc_parameters_end": (C.c_int, [H, dp]),
        "amc_pg_estimate": (C.c_int, [H, C.c_int, ip, C.c_int, dp]),
        "amc_pg_accumulate": (C.c_int, [H, C.c_int, ip, C.c_int]),
        "amc_pg_update": (C.c_int, [H, C.c_int, ip, ip, dp, dp]),
        "amc_pg_get_accumulated": (C.c_int, [H, C.c_int, ip, dp]),
        "amc_pg_set_accumulated": (C.c_int, [H, C.c_int, ip, dp]),
        "amc_pgmc_steps": (C.c_int, [H, C.c_int64, C.c_int, ip, C.c_int, C.c_int, ip, dp, dp]),
        "amc_pgmc_steps_reduce_begin": (C.c_int, [H, C.c_int64, C.c_int, ip, C.c_int, C.c_int, ip, dp, dp]),
        "amc_sync": (C.c_int, [H]),
        "amc_get_stream": (C.c_int, [H, C.POINTER(C.c_void_p)]),
        "amc_timing_begin": (C.c_int, [H]),
        "amc_timing_end": (C.c_int, [H, dp]),
        "amc_timing_mark": (C.c_int, [H]),
        "amc_comm_unique_id": (C.c_int, [C.c_void_p]),
        "amc_comm_init": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p]),
        "amc_allreduce_sum": (C.c_int, [H, dp, C.c_int]),
        "amc_comm_destroy": (C.c_int, [H]),
        "amc_comm_info": (C.c_int, [H, ip, ip, ip, sp, C.c_int]),
        "amc_runtime_info": (C.c_int, [ip, sp, C.c_int]),
        "amc_selftest_math": (C.c_int, [C.c_int, C.c_int, dp, dp, dp, C.c_int64]),
        "amc_selftest_accept_filter": (C.c_int, [C.c_int, C.c_float, C.c_float, dp]),
        "amc_selftest_filter_argument": (C.c_int, [C.c_int, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_float), C.c_int64]),
        "amc_selftest_philox": (C.c_int, [C.c_int, C.c_uint64, u64p, u64p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_int64]),
        "amc_set_reduce_columns": (C.c_int, [H, C.c_int]),
        "amc_parameters_end_all": (C.c_int, [H, dp, C.c_int]),
        "amc_selftest_wave_totals": (C.c_int, [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "amc_selftest_staged_tables": (C.c_int, [C.c_int, dp]),
        "amc_set_ladder": (C.c_int, [H, C.c_int]),
        "amc_exchange": (C.c_int, [H, C.c_int64]),
        "amc_sweep_exchange": (C.c_int, [H, C.c_int64, C.c_int64]),
        "amc_exchange_counters": (C.c_int, [H, i64p, i64p]),
        "amc_set_exchange_counters": (C.c_int, [H, i64p, i64p]),
        "amc_get_exchange_step": (C.c_int, [H, u64p]),
        "amc_set_exchange_step": (C.c_int, [H, C.c_uint64]),
        "amc_histogram_rungs": (C.c_int, [H, C.c_double, C.c_double, C.c_int, u64p]),
        "amc_reduce_rungs_exact": (C.c_int, [H, C.c_int, dp]),
        "amc_bridge_accumulate": (C.c_int, [H, C.c_int]),
        "amc_bridge_fetch": (C.c_int, [H, dp, u64p, C.c_int]),
        "amc_set_bridge": (C.c_int, [H, dp, C.c_uint64]),
        "amc_corr_mark": (C.c_int, [H, C.c_int]),
        "amc_corr_sample": (C.c_int, [H]),
        "amc_corr_fetch": (C.c_int, [H, dp, u64p, C.c_int, ip, ip]),
        "amc_corr_download_origin": (C.c_int, [H, dp]),
        "amc_set_corr": (C.c_int, [H, C.c_int, dp, dp, u64p, C.c_int]),
        "amc_corr_clear": (C.c_int, [H]),
        "amc_energy_histogram_accumulate": (C.c_int, [H, C.c_double, C.c_double, C.c_int]),
        "amc_energy_histogram_fetch": (C.c_int, [H, u64p, C.c_int64, ip, ip, dp, dp, u64p, C.c_int]),
        "amc_set_energy_histogram": (C.c_int, [H, C.c_double, C.c_double, C.c_int, u64p, C.c_uint64]),
        "amc_chain_stats_accumulate": (C.c_int, [H, C.c_int, C.c_int]),
        "amc_chain_stats_fetch": (C.c_int, [H, dp, C.c_int, u64p, ip, ip]),
        "amc_chain_stats_download": (C.c_int, [H, dp]),
        "amc_set_chain_stats": (C.c_int, [H, C.c_int, u64p, dp]),
        "amc_chain_stats_clear": (C.c_int, [H]),
        "amc_set_blocks": (C.c_int, [H, C.c_int, C.c_int64]),
        "amc_bridge_fetch_blocks": (C.c_int, [H, dp, C.c_int, ip, u64p, C.c_int]),
        "amc_corr_fetch_blocks": (C.c_int, [H, dp, u64p, C.c_int, ip, ip, ip]),
        "amc_set_bridge_blocks": (C.c_int, [H, dp, C.c_int, C.c_uint64]),
        "amc_set_corr_blocks": (C.c_int, [H, C.c_int, dp, dp, u64p, C.c_int, C.c_int]),
        "amc_energy_histogram_accumulate_blocks": (C.c_int, [H, C.c_double, C.c_double, C.c_int]),
        "amc_energy_histogram_fetch_blocks": (C.c_int, [H, u64p, C.c_int64, ip, ip, ip, dp, dp, u64p, C.c_int]),
        "amc_set_energy_histogram_blocks": (C.c_int, [H, C.c_double, C.c_double, C.c_int, u64p, C.c_int, C.c_uint64]),
        "amc_energy_moments_accumulate": (C.c_int, [H, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double]),
        "amc_energy_moments_fetch": (C.c_int, [H, u64p, i64p, C.c_int64, C.c_int64, ip, ip, ip, dp, dp, ip, dp, u64p, C.c_int]),
        "amc_set_energy_moments": (C.c_int, [H, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, u64p, i64p, C.c_uint64]),
        "amc_energy_moments_accumulate_blocks": (C.c_int, [H, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double]),
        "amc_energy_moments_fetch_blocks": (C.c_int, [H, u64p, i64p, C.c_int64, C.c_int64, ip, ip, ip, ip, dp, dp, ip, dp, u64p, C.c_int]),
        "amc_set_energy_moments_blocks": (C.c_int, [H, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, u64p, i64p, C.c_int, C.c_uint64]),
        "amc_set_tracking": (C.c_int, [H, C.c_int]),
        "amc_download_labels": (C.c_int, [H, C.POINTER(C.c_uint8)]),
        "amc_upload_labels": (C.c_int, [H, C.POINTER(C.c_uint8)]),
        "amc_flow_rungs": (C.c_int, [H, u64p]),
        "amc_tracking_counters": (C.c_int, [H, i64p, i64p]),
        "amc_set_tracking_counters": (C.c_int, [H, C.c_int64, C.c_int64]),
        "amc_set_rung_sigma": (C.c_int, [H, dp, C.c_int]),
        "amc_get_rung_sigma": (C.c_int, [H, dp, C.c_int]),
        "amc_respace_ladder": (C.c_int, [H, C.c_int, C.c_double, C.c_double, u64p]),
        "amc_respace_status": (C.c_int, [H, ip, i64p]),
        "amc_set_respaced": (C.c_int, [H, C.c_int64]),
        "amc_get_ladder": (C.c_int, [H, dp]),
        "amc_rung_counter_totals": (C.c_int, [H, i64p, i64p]),
        "amc_tune_rung_sigma": (C.c_int, [H, C.c_double, C.c_double, C.c_int64, C.c_double, C.c_double, i64p]),
        "amc_tune_status": (C.c_int, [H, ip, C.c_int, i64p]),
        "amc_set_tuned": (C.c_int, [H, C.c_int64]),
        "amc_rung_window_counts": (C.c_int, [H, i64p, i64p]),
        "amc_rung_window_restart": (C.c_int, [H]),
        "amc_rung_window_base": (C.c_int, [H, i64p, i64p]),
        "amc_set_rung_window_base": (C.c_int, [H, i64p, i64p]),
        "amc_anneal": (C.c_int, [H, C.c_double]),
        "amc_anneal_fetch": (C.c_int, [H, u64p, C.c_int, ip, C.c_int]),
        "amc_set_anneal_records": (C.c_int, [H, u64p, C.c_int]),
        "amc_get_anneal_step": (C.c_int, [H, u64p]),
        "amc_set_anneal_step": (C.c_int, [H, C.c_uint64]),
        "amc_get_beta": (C.c_int, [H, dp]),
        "amc_set_beta": (C.c_int, [H, C.c_double]),
        "amc_anneal_next_beta": (C.c_int, [H, C.c_double, C.c_double, C.c_int, dp, u64p, u64p]),
        "amc_set_anneal_families": (C.c_int, [H, C.c_int]),
        "amc_anneal_family_stats": (C.c_int, [H, u64p, u64p, u64p]),
        "amc_download_families": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "amc_upload_families": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "amc_set_anneal_blocks": (C.c_int, [H, C.c_int, C.c_int64]),
        "amc_anneal_fetch_blocks": (C.c_int, [H, u64p, C.c_int, ip, ip, C.c_int]),
        "amc_set_anneal_block_records": (C.c_int, [H, u64p, C.c_int, C.c_int]),
        "amc_anneal_block_counts": (C.c_int, [H, u64p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    SIGNATURES.update(sig)
    _lib = lib
    return lib


def runtime_info() -> dict:
    """The HIP runtime libamc.so is bound to in this process: hipRuntimeGetVersion and the file it came from."""
    v = C.c_int(0)
    path = C.create_string_buffer(1024)
    _check(load().amc_runtime_info(C.byref(v), path, 1024))
    return {"hip_runtime_version": v.value, "hip_runtime": path.value.decode()}


def _check(rc: int) -> None:
    if rc != 0:
        msg = load().amc_last_error()
        raise AmcError(f"amc error {rc}: {msg.decode() if msg else '?'}")


def model_check(sample, logq, dlogq=None, perform=None, invert=None, *, n_params: int = 1, potential: Optional[str] = None,
                reward: Optional[str] = None) -> str:
    """Compile-only check of a script-defined model (no GPU needed; amc_model_check): one policy -- strings, `dlogq` a string, a
    list of n_params strings or None (forward-mode differentiation of logq) -- or a pool of classes -- lists with one entry per
    class, None entries where a class has no expression of that kind.  Returns the compiler log."""
    many = isinstance(sample, (list, tuple))
    n_classes = len(sample) if many else 1

    def col(v, n):
        if v is None:
            return None
        items = list(v) if isinstance(v, (list, tuple)) else [v]
        assert len(items) == n, (items, n)
        return (C.c_char_p * n)(*[None if e is None else str(e).encode() for e in items])
    n_d = n_classes if many else int(n_params)
    buf = C.create_string_buffer(8192)
    lib = load()
    _check(lib.amc_model_check(int(n_params), n_classes, None if potential is None else str(potential).encode(),
                               None if reward is None else str(reward).encode(), col(sample, n_classes), col(logq, n_classes),
                               col(dlogq, n_d), col(perform, n_classes), col(invert, n_classes), buf, len(buf)))
    return buf.value.decode(errors="replace")


def device_count() -> int:
    n = C.c_int(0)
    rc = load().amc_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def potential_check(expr: str) -> str:
    """Compile-only check of a custom potential expression (no GPU needed); returns the compiler log, raises
    AmcError with the first diagnostics when the expression does not compile."""
    buf = C.create_string_buffer(8192)
    _check(load().amc_potential_check(str(expr).encode(), buf, len(buf)))
    return buf.value.decode(errors="replace")


_POINTERS = {np.dtype(t): C.POINTER(c) for t, c in (
    (np.float64, C.c_double), (np.float32, C.c_float), (np.int64, C.c_int64), (np.uint64, C.c_uint64), (np.int32, C.c_int),
    (np.uint32, C.c_uint32), (np.uint8, C.c_uint8))}


def _ptr(a: Optional[np.ndarray]):
    """The pointer to a contiguous array's data, typed after its dtype as the entry point's prototype has it (None: NULL)."""
    return None if a is None else a.ctypes.data_as(_POINTERS[a.dtype])


def _carray(ctype, values, n: int):
    """``values`` as a ctypes array of at least one entry: the learn_ids / kinds (c_int) and hyperparameters (c_double) of amc_pg_*."""
    conv = float if ctype is C.c_double else int
    return (ctype * max(n, 1))(*[conv(v) for v in values])


def _u64_property(name: str):
    """The step index amc_get_<name> / amc_set_<name> as a property."""
    getter, setter = "amc_get_" + name, "amc_set_" + name

    def get(self) -> int:
        t = C.c_uint64(0)
        _check(getattr(self._lib, getter)(self._h, C.byref(t)))
        return t.value

    def put(self, t: int) -> None:
        _check(getattr(self._lib, setter)(self._h, int(t)))
    return property(get, put)


# ---- reproducible sums (include/amc.h "Reproducible sums"): records are rows of AMC_XSUM_WORDS doubles -----------------
def xsum_merge(into: np.ndarray, other: np.ndarray) -> np.ndarray:
    """into[i] += other[i] for records of shape (n, AMC_XSUM_WORDS); exact (integers), so the order of merges is immaterial."""
    a = np.ascontiguousarray(into, dtype=np.float64).reshape(-1, AMC_XSUM_WORDS).copy()
    b = np.ascontiguousarray(other, dtype=np.float64).reshape(-1, AMC_XSUM_WORDS)
    if a.shape != b.shape:
        raise AmcError(f"xsum_merge: record arrays of shapes {a.shape} and {b.shape}")
    _check(load().amc_xsum_merge(_ptr(a), _ptr(b), a.shape[0]))
    return a


def xsum_round(records: np.ndarray) -> np.ndarray:
    """The Float64 of each record: the integer total rounded once."""
    a = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, AMC_XSUM_WORDS)
    out = np.empty(a.shape[0], dtype=np.float64)
    _check(load().amc_xsum_round(_ptr(a), a.shape[0], _ptr(out)))
    return out


def xsum_plain(values) -> np.ndarray:
    """Records that hold plain numbers (counts: integers, exact under +)."""
    v = np.atleast_1d(np.asarray(values, dtype=np.float64))
    rec = np.zeros((v.size, AMC_XSUM_WORDS))
    rec[:, 0] = 3.0
    rec[:, 11] = v
    return rec


def comm_library_forced() -> bool:
    """True when AMC_RCCL_LIBRARY replaced librccl in this process (a site's own build, or the tests' stand-in)."""
    f = C.c_int(0)
    _check(load().amc_comm_library_forced(C.byref(f)))
    return bool(f.value)


class HipEngine:
    """One amc_handle: the device-resident shard of the chain ensemble.

    Mirrors what the reference's ``Metropolis`` object owns (pools, seed, rngs,
    sweepstep: src/metropolis.jl:232-239), SoA on one MI355X.
    """

    def __init__(self, *, n_chains: int, chain_offset: int = 0, n_chains_global: Optional[int] = None,
                 potential="harmonic", beta: float = 1.0, sigma: Sequence[float] = (1.0,),
                 weight: Sequence[float] = (1.0,), seed: int = 1, sweepstep: int = 1,
                 per_chain_counters: bool = True, device: int = 0, stream: Optional[int] = None,
                 reward_expr: Optional[str] = None, dtype: str = "f64", scale_expr: Optional[str] = None,
                 proposal: Optional[Sequence[Optional[str]]] = None, n_params: int = 1,
                 classes: Optional[Sequence[Sequence[Optional[str]]]] = None, class_of_move: Optional[Sequence[int]] = None,
                 param_dtype: str = "f64"):
        """``param_dtype`` "f32" (with ``dtype`` "f32"): the all-Float32 model -- sigma, the normal variate and the displacement
        are Float32 (amc_config.param_dtype); ``sigma`` must then hold Float32 values.  Sweeps with the built-in policy only.
        ``n_params`` > 1 (with ``proposal``): a policy with several parameters (amc_create_vector_policy_model) -- the
        expressions see theta0 .. theta{P-1}, ``proposal[2]`` is the list of the P partials of logq (or None), and ``sigma``
        holds one parameter VECTOR per move.
        ``classes`` (with ``class_of_move``): a pool that MIXES policy / action types (amc_create_mixed_model) -- one
        (sample, logq, dlogq or None[, perform, invert]) per class, ``class_of_move[k]`` the class move k uses."""
        lib = load()
        if str(dtype) not in STATE_DTYPES:
            raise AmcError(f"unknown state dtype {dtype!r}; one of {sorted(STATE_DTYPES)}")
        self.dtype = "f32" if STATE_DTYPES[str(dtype)] else "f64"
        if str(param_dtype) not in STATE_DTYPES:
            raise AmcError(f"unknown param_dtype {param_dtype!r}; one of {sorted(STATE_DTYPES)}")
        self.param_dtype = "f32" if STATE_DTYPES[str(param_dtype)] else "f64"
        expr = getattr(potential, "expr", None)        # system.CustomPotential: a C expression in x
        if expr is None and potential not in POTENTIALS:
            raise AmcError(f"unknown potential {potential!r}; the HIP engine offers {sorted(POTENTIALS)} "
                           "and CustomPotential(expr)")
        self.n_chains = int(n_chains)
        self.n_moves = len(sigma)
        self.n_rungs = 0                       # rungs per ladder (set_ladder sets it; 0: no ladder)
        self.n_params = int(n_params)
        self.gd_stride = 2 + 2 * self.n_params + self.n_params ** 2          # AMC_GD_STRIDE_P
        if self.n_params != 1 and proposal is None:
            raise AmcError("n_params > 1 needs a script-defined proposal (sample, logq, [dlogq ...])")
        theta = None
        if self.n_params > 1:
            theta = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in sigma]
            if any(v.size != self.n_params for v in theta):
                raise AmcError(f"sigma must hold one vector of {self.n_params} parameters per move")
            sigma = [1.0] * self.n_moves          # parameter 0 at creation; the vectors follow through amc_set_parameters
        self.per_chain_counters = bool(per_chain_counters) or self.n_moves > 1
        self._sigma = (C.c_double * self.n_moves)(*[float(s) for s in sigma])
        self._weight = (C.c_double * self.n_moves)(*[float(w) for w in weight])
        cfg = AmcConfig()
        cfg.struct_size = C.sizeof(AmcConfig)
        cfg.device = int(device)
        cfg.n_chains = self.n_chains
        cfg.chain_offset = int(chain_offset)
        cfg.n_chains_global = int(n_chains_global if n_chains_global is not None else chain_offset + n_chains)
        cfg.potential = AMC_POTENTIAL_CUSTOM if expr is not None else POTENTIALS[potential]
        cfg.n_moves = self.n_moves
        cfg.beta = float(beta)
        cfg.sigma = self._sigma
        cfg.weight = self._weight
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.sweepstep = int(sweepstep)
        cfg.per_chain_counters = 1 if per_chain_counters else 0
        cfg.stream = stream
        cfg.state_dtype = STATE_DTYPES[self.dtype]
        cfg.param_dtype = STATE_DTYPES[self.param_dtype]
        self._lib = lib
        self._h = C.c_void_p()
        enc = lambda t: None if t is None else str(t).encode()
        if classes is not None:
            if proposal is not None or scale_expr is not None or self.n_params != 1:
                raise AmcError("classes cannot be combined with proposal / scale_expr / n_params > 1")
            if class_of_move is None or len(class_of_move) != self.n_moves:
                raise AmcError("class_of_move must name one class per move")
            cl = [tuple((list(c) + [None] * 4)[:5]) for c in classes]
            n = len(cl)
            arr = lambda i, need: ((C.c_char_p * n)(*[enc(c[i]) for c in cl]) if need else None)
            have_d = any(c[2] is not None for c in cl)       # a class without one has its logq differentiated by the engine (NULL entry)
            com = (C.c_int * self.n_moves)(*[int(v) for v in class_of_move])
            _check(lib.amc_create_mixed_model(C.byref(cfg), n, com, enc(expr), enc(reward_expr), arr(0, True), arr(1, True), arr(2, have_d),
                                              arr(3, any(c[3] is not None for c in cl)), arr(4, any(c[4] is not None for c in cl)),
                                              C.byref(self._h)))
        elif proposal is not None:
            # script-defined sample_action! / log_proposal_density (/ its sigma-derivative) and, optionally, the action's
            # perform_action! / invert_action!: (sample, logq, dlogq or None[, perform, invert])
            if scale_expr is not None:
                raise AmcError("a script-defined proposal and a ScaledGaussian scale cannot be combined")
            sample, logq, dlogq, perform, invert = (list(proposal) + [None] * 4)[:5]
            if self.n_params > 1:
                partials = None
                if dlogq is not None:
                    if isinstance(dlogq, (str, bytes)) or len(dlogq) != self.n_params:
                        raise AmcError(f"proposal[2] must list the {self.n_params} partial derivatives of logq (or be None)")
                    partials = (C.c_char_p * self.n_params)(*[enc(d) for d in dlogq])
                _check(lib.amc_create_vector_policy_model(C.byref(cfg), self.n_params, enc(expr), enc(reward_expr), enc(sample),
                                                          enc(logq), partials, enc(perform), enc(invert), C.byref(self._h)))
                for k, v in enumerate(theta):
                    self.set_parameters(k, v)
            else:
                _check(lib.amc_create_action_model(C.byref(cfg), enc(expr), enc(reward_expr), enc(sample), enc(logq), enc(dlogq),
                                                   enc(perform), enc(invert), C.byref(self._h)))
        elif scale_expr is not None:
            # script-defined policy of the Gaussian-displacement family: proposal width sigma * scale(x)
            _check(lib.amc_create_policy_model(C.byref(cfg), enc(expr), enc(reward_expr), enc(scale_expr), C.byref(self._h)))
        elif reward_expr is not None:
            # script-defined reward(action, system) (gradients.jl:20): an expression in delta and the new position x
            _check(lib.amc_create_model(C.byref(cfg), enc(expr), enc(reward_expr), C.byref(self._h)))
        elif expr is not None:
            _check(lib.amc_create_custom(C.byref(cfg), enc(expr), C.byref(self._h)))
        else:
            _check(lib.amc_create(C.byref(cfg), C.byref(self._h)))

    # -- lifetime --------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.amc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state -----------------------------------------------------------------
    def upload_state(self, x: np.ndarray, beta: Optional[np.ndarray] = None) -> None:
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.n_chains,):
            raise AmcError(f"upload_state: x has shape {x.shape}, expected ({self.n_chains},)")
        if beta is not None:
            beta = np.ascontiguousarray(beta, dtype=np.float64)
            if beta.shape != (self.n_chains,):
                raise AmcError("upload_state: beta must have one entry per chain")
        _check(self._lib.amc_upload_state(self._h, _ptr(x), _ptr(beta)))

    def init_uniform(self, lo: float, hi: float) -> None:
        _check(self._lib.amc_init_uniform(self._h, float(lo), float(hi)))

    def download_state(self, want_e: bool = True):
        x = np.empty(self.n_chains, dtype=np.float64)
        e = np.empty(self.n_chains, dtype=np.float64) if want_e else None
        _check(self._lib.amc_download_state(self._h, _ptr(x), _ptr(e)))
        return x, e

    def _rungs(self) -> int:
        return max(self.n_rungs, 1)                    # R as array shapes need it: at least 1, ladder or none

    def _i64_pair(self, fn, shape):
        """What an entry point ``fn(handle, int64 *, int64 *)`` writes, as two arrays of ``shape``."""
        acc = np.zeros(shape, dtype=np.int64)
        tot = np.zeros(shape, dtype=np.int64)
        _check(fn(self._h, _ptr(acc), _ptr(tot)))
        return acc, tot

    def download_counters(self):
        return self._i64_pair(self._lib.amc_download_counters, (self.n_moves, self.n_chains))

    def counter_totals(self):
        return self._i64_pair(self._lib.amc_counter_totals, self.n_moves)

    def upload_counters(self, accepted: np.ndarray, total: Optional[np.ndarray] = None) -> None:
        a = np.ascontiguousarray(accepted, dtype=np.int64).reshape(self.n_moves, self.n_chains)
        t = None if total is None else np.ascontiguousarray(total, dtype=np.int64).reshape(self.n_moves, self.n_chains)
        _check(self._lib.amc_upload_counters(self._h, _ptr(a), _ptr(t)))

    def set_counter_totals(self, accepted: int, steps_counted: int) -> None:
        a = np.array([int(accepted)], dtype=np.int64)
        _check(self._lib.amc_set_counter_totals(self._h, _ptr(a), int(steps_counted)))

    def histogram(self, lo: float, hi: float, n_bins: int) -> np.ndarray:
        """counts[n_bins + 3]: the bins of [lo, hi), then below lo, at/above hi, NaN (this shard only)."""
        out = np.zeros(int(n_bins) + 3, dtype=np.uint64)
        _check(self._lib.amc_histogram(self._h, float(lo), float(hi), int(n_bins), _ptr(out)))
        return out

    def histogram_accumulate(self, lo: float, hi: float, n_bins: int) -> None:
        """Add the histogram of the positions as of this point of the stream to the running one on the device (asynchronous)."""
        _check(self._lib.amc_histogram_accumulate(self._h, float(lo), float(hi), int(n_bins)))

    def histogram_fetch(self, n_bins: int, reset: bool = True) -> np.ndarray:
        out = np.zeros(int(n_bins) + 3, dtype=np.uint64)
        _check(self._lib.amc_histogram_fetch(self._h, _ptr(out), int(n_bins), 1 if reset else 0))
        return out

    def download_strided(self, first: int, stride: int, count: int) -> np.ndarray:
        out = np.empty(int(count), dtype=np.float64)
        _check(self._lib.amc_download_strided(self._h, int(first), int(stride), int(count), _ptr(out)))
        return out

    # the Philox step indices of the sweeps, the estimator, the exchange steps and the annealing steps
    step = _u64_property("step")
    estimator_step = _u64_property("estimator_step")
    exchange_step = _u64_property("exchange_step")
    anneal_step = _u64_property("anneal_step")

    # -- hot path ----------------------------------------------------------------
    def sweep(self, n_sweeps: int = 1) -> None:
        _check(self._lib.amc_sweep(self._h, int(n_sweeps)))

    def reduce(self) -> np.ndarray:
        out = np.empty(AMC_RED_HEADER + self.n_moves, dtype=np.float64)
        _check(self._lib.amc_reduce(self._h, _ptr(out)))
        return out

    REDUCE_E, REDUCE_X, REDUCE_XX, REDUCE_ALL = AMC_REDUCE_E, AMC_REDUCE_X, AMC_REDUCE_XX, AMC_REDUCE_ALL

    def set_reduce_columns(self, columns: int) -> None:
        """Which of sum e / sum x / sum x^2 the reductions begun from now on form (amc_set_reduce_columns; REDUCE_* bits).  A
        sum that is not formed reads NaN."""
        _check(self._lib.amc_set_reduce_columns(self._h, int(columns)))

    def reduce_begin(self) -> None:
        """Enqueue the reduction; sweeps queued afterwards keep running while the host does other work."""
        _check(self._lib.amc_reduce_begin(self._h))

    def sweep_reduce_begin(self, n_sweeps: int = 1) -> None:
        """n sweeps, then the callback reduction of the resulting state (fused into the last launch when possible)."""
        _check(self._lib.amc_sweep_reduce_begin(self._h, int(n_sweeps)))

    def reduce_end(self) -> np.ndarray:
        out = np.empty(AMC_RED_HEADER + self.n_moves, dtype=np.float64)
        _check(self._lib.amc_reduce_end(self._h, _ptr(out)))
        return out

    def reduce_end_exact(self):
        """The oldest reduction in flight as records, shape (AMC_RED_HEADER + K, AMC_XSUM_WORDS), and the MH steps counted per
        chain when it was begun.  What shards exchange (sharding.allreduce_xsum); ``reduce_records_value`` turns merged
        records into the numbers reduce_end() returns."""
        rec = np.zeros((AMC_RED_HEADER + self.n_moves, AMC_XSUM_WORDS), dtype=np.float64)
        steps = C.c_uint64(0)
        _check(self._lib.amc_reduce_end_exact(self._h, _ptr(rec), C.byref(steps)))
        return rec, int(steps.value)

    def reduce_exact(self):
        self.reduce_begin()
        return self.reduce_end_exact()

    def reduce_records_value(self, records: np.ndarray, steps_counted: int) -> np.ndarray:
        """Merged records -> the sums (layout of amc_reduce).  A K = 1 engine without per-chain counters carries the pool-wide
        accepted TOTAL in the ratio record: every chain has the same total_calls, the ratio sum is that total / steps."""
        out = xsum_round(records)
        out[np.asarray(records).reshape(-1, AMC_XSUM_WORDS)[:, 0] == 0.0] = np.nan      # an empty record: a sum nobody asked for
        if self.n_moves == 1 and not self.per_chain_counters:
            with np.errstate(invalid="ignore", divide="ignore"):
                out[AMC_RED_HEADER] = out[AMC_RED_HEADER] / np.float64(steps_counted)   # 0/0 = NaN before the first step
        return out

    def set_parameters(self, k: int, p: Sequence[float]) -> None:
        a = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
        _check(self._lib.amc_set_parameters(self._h, int(k), _ptr(a), int(a.size)))

    def get_parameters(self, k: int) -> np.ndarray:
        a = np.empty(self.n_params, dtype=np.float64)
        _check(self._lib.amc_get_parameters(self._h, int(k), _ptr(a), self.n_params))
        return a

    def parameters_begin(self) -> None:
        """Queue a read of every move's sigma as of this point of the stream (amc_parameters_begin); fetch with parameters_end()."""
        _check(self._lib.amc_parameters_begin(self._h))

    def parameters_end(self) -> np.ndarray:
        """sigma[K] -- for a policy with several parameters all of them, shape (K, P)."""
        if self.n_params > 1:
            a = np.empty((self.n_moves, self.n_params), dtype=np.float64)
            _check(self._lib.amc_parameters_end_all(self._h, _ptr(a), a.size))
            return a
        a = np.empty(self.n_moves, dtype=np.float64)
        _check(self._lib.amc_parameters_end(self._h, _ptr(a)))
        return a

    def pg_estimate(self, learn_ids: Sequence[int], q_batch: int) -> np.ndarray:
        n = len(learn_ids)
        out = np.zeros((n, self.gd_stride), dtype=np.float64)
        _check(self._lib.amc_pg_estimate(self._h, n, _carray(C.c_int, learn_ids, n), int(q_batch), _ptr(out)))
        return out

    def pg_estimate_exact(self, learn_ids: Sequence[int], q_batch: int) -> np.ndarray:
        """The same fold as records, shape (n_learn, AMC_GD_STRIDE, AMC_XSUM_WORDS): what shards exchange."""
        n = len(learn_ids)
        out = np.zeros((n, self.gd_stride, AMC_XSUM_WORDS), dtype=np.float64)
        _check(self._lib.amc_pg_estimate_exact(self._h, n, _carray(C.c_int, learn_ids, n), int(q_batch), _ptr(out)))
        return out

    def sweep_launches(self, n_launches: int) -> None:
        """n make_step!s as n launches of one sweep each, queued by one call (amc_sweep_launches)."""
        _check(self._lib.amc_sweep_launches(self._h, int(n_launches)))

    def pg_route(self, n_learn: int, q_batch: int = 1, fused: bool = False):
        """(one_launch, why): whether an estimator call over n_learn learnable moves takes them all in ONE launch -- with
        ``fused``: whether the whole time step (sweep + estimator + update) is one launch -- and, for a pool of several classes
        whose several-move kernel form the run-time compiler fails on, what the compiler said (the calls then take one launch per
        move: same bits).  ``pg_route_code`` returns amc_pg_route's own answer (2 / 1 / 0)."""
        code, why = self.pg_route_code(n_learn, q_batch, fused)
        return (code == 2 if fused else code >= 1), why

    def pg_route_code(self, n_learn: int, q_batch: int = 1, fused: bool = False):
        why = C.create_string_buffer(2048)
        rc = self._lib.amc_pg_route(self._h, int(n_learn), int(q_batch), int(bool(fused)), why, len(why))
        if rc < 0:
            _check(rc)
        return int(rc), why.value.decode(errors="replace")

    def pg_accumulate(self, learn_ids: Sequence[int], q_batch: int) -> None:
        """Estimator step kept on the device: gradients_data[k] += gd (asynchronous)."""
        n = len(learn_ids)
        _check(self._lib.amc_pg_accumulate(self._h, n, _carray(C.c_int, learn_ids, n), int(q_batch)))

    def pg_update(self, learn_ids: Sequence[int], kinds: Sequence[int], hyper0: Sequence[float],
                  hyper1: Sequence[float]) -> None:
        """average -> learning_step! -> reset on the device; sigma and its table are refreshed in place."""
        n = len(learn_ids)
        _check(self._lib.amc_pg_update(self._h, n, _carray(C.c_int, learn_ids, n), _carray(C.c_int, kinds, n), _carray(C.c_double, hyper0, n),
                                       _carray(C.c_double, hyper1, n)))

    def pgmc_steps(self, n_steps: int, learn_ids: Sequence[int], q_batch: int, kinds: Optional[Sequence[int]] = None,
                   hyper0: Sequence[float] = (), hyper1: Sequence[float] = (), reduce_begin: bool = False) -> None:
        """n x [sweep(1); pg_accumulate; pg_update if kinds is given] enqueued by one call (asynchronous).
        ``reduce_begin``: followed by reduce_begin() of the state the last step leaves -- the callback sums then ride in that
        step's launch (amc_pgmc_steps_reduce_begin); fetch them with reduce_end()."""
        n = len(learn_ids)
        ids = (C.c_int * max(n, 1))(*[int(i) for i in learn_ids])           # (the step loop's call: _carray spelt out)
        do_update = kinds is not None
        kd = (C.c_int * max(n, 1))(*[int(k) for k in (kinds or [0] * n)])
        h0 = (C.c_double * max(n, 1))(*[float(v) for v in (hyper0 if do_update else [0.0] * n)])
        h1 = (C.c_double * max(n, 1))(*[float(v) for v in (hyper1 if do_update else [0.0] * n)])
        fn = self._lib.amc_pgmc_steps_reduce_begin if reduce_begin else self._lib.amc_pgmc_steps
        _check(fn(self._h, int(n_steps), n, ids, int(q_batch), 1 if do_update else 0, kd, h0, h1))

    def pg_get_accumulated(self, learn_ids: Sequence[int]) -> np.ndarray:
        n = len(learn_ids)
        out = np.zeros((n, self.gd_stride), dtype=np.float64)
        _check(self._lib.amc_pg_get_accumulated(self._h, n, _carray(C.c_int, learn_ids, n), _ptr(out)))
        return out

    def pg_set_accumulated(self, learn_ids: Sequence[int], rows: np.ndarray) -> None:
        """Resume: replace the device-resident gradients_data of the moves learn_ids by rows[n][5] (j, grad_j, grad_logq, g, n)."""
        n = len(learn_ids)
        a = np.ascontiguousarray(rows, dtype=np.float64).reshape(n, self.gd_stride)
        _check(self._lib.amc_pg_set_accumulated(self._h, n, _carray(C.c_int, learn_ids, n), _ptr(a)))

    # -- population annealing (include/amc.h) ---------------------------------------
    def anneal(self, beta_new: float) -> None:
        """One annealing step (asynchronous): the shared beta moves to ``beta_new`` and the whole ensemble is resampled in proportion
        to exp(-(beta_new - beta) e)."""
        _check(self._lib.amc_anneal(self._h, float(beta_new)))

    def anneal_records(self, reset: bool = False) -> np.ndarray:
        """The records of the annealing steps in the log, shape (n, 8) uint64: status, bits of beta before / after, bits of a_max, T_w,
        U, n_parents, max_children (synchronises); ``reset`` empties the log."""
        n = C.c_int(0)
        _check(self._lib.amc_anneal_fetch(self._h, None, 0, C.byref(n), 0))
        out = np.zeros((n.value, AMC_ANNEAL_RECORD_WORDS), dtype=np.uint64)
        _check(self._lib.amc_anneal_fetch(self._h, _ptr(out), n.value, C.byref(n), 1 if reset else 0))
        return out

    def set_anneal_records(self, records) -> None:
        rec = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, AMC_ANNEAL_RECORD_WORDS)
        _check(self._lib.amc_set_anneal_records(self._h, _ptr(rec), int(rec.shape[0])))

    @property
    def beta(self) -> float:
        """The shared beta as the launches queued from now on use it (amc_anneal moves it)."""
        b = C.c_double(0.0)
        _check(self._lib.amc_get_beta(self._h, C.byref(b)))
        return b.value

    @beta.setter
    def beta(self, b: float) -> None:
        _check(self._lib.amc_set_beta(self._h, float(b)))

    def anneal_next_beta(self, beta_limit: float, target: float, rounds: int = 6):
        """(beta_new, diag, trace): the largest step from the shared beta towards ``beta_limit`` whose reweighting keeps ESS / M at or
        above ``target``, searched on the device in ``rounds`` rounds of 8 candidates (rounds = 6 resolves 8^-6 of the span);
        synchronises once.  Nothing moves: hand ``beta_new`` to anneal().  diag: 8 uint64 words (status, rounds decided, bits of the
        step, rho at the low end, bits of the high end, rho there, bits of the largest / smallest -e); trace: (rounds, 8, 3) uint64, every
        candidate's S1, S2h, S2l."""
        b = C.c_double(0.0)
        diag = np.zeros(AMC_ANNEAL_SEARCH_WORDS, dtype=np.uint64)
        trace = np.zeros((max(int(rounds), 0), AMC_ANNEAL_SEARCH_CANDIDATES, 3), dtype=np.uint64)
        _check(self._lib.amc_anneal_next_beta(self._h, float(beta_limit), float(target), int(rounds), C.byref(b), _ptr(diag),
                                              _ptr(trace) if trace.size else None))
        return b.value, diag, trace

    def set_anneal_families(self, on: bool = True) -> None:
        _check(self._lib.amc_set_anneal_families(self._h, 1 if on else 0))

    def anneal_family_stats(self):
        """(families with a member, sum of n_f^2, largest n_f): exact integers (synchronises)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self._lib.amc_anneal_family_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def download_families(self) -> np.ndarray:
        out = np.empty(self.n_chains, dtype=np.uint32)
        _check(self._lib.amc_download_families(self._h, _ptr(out)))
        return out

    def upload_families(self, families) -> None:
        fam = np.ascontiguousarray(families, dtype=np.uint32)
        if fam.shape != (self.n_chains,):
            raise AmcError(f"upload_families: one id per chain ({self.n_chains})")
        _check(self._lib.amc_upload_families(self._h, _ptr(fam)))

    def set_anneal_blocks(self, n_blocks: int, chunk: int = 0) -> None:
        """The partition into blocks of families, block of chain c = (fam[c] // chunk) % n_blocks (0: off; chunk = 0: ceil(M / B)); needs
        families on.  Every annealing step from then on appends a block record."""
        _check(self._lib.amc_set_anneal_blocks(self._h, int(n_blocks), int(chunk)))

    def anneal_block_records(self, reset: bool = False) -> np.ndarray:
        """The block records in the log, shape (n, 2, B) uint64: n_b before the resampling, then T_b = the sum of W over block b
        (synchronises); ``reset`` empties this log (not the records' log)."""
        n, B = C.c_int(0), C.c_int(0)
        _check(self._lib.amc_anneal_fetch_blocks(self._h, None, 0, C.byref(n), C.byref(B), 0))
        out = np.zeros((n.value, 2, B.value), dtype=np.uint64)
        _check(self._lib.amc_anneal_fetch_blocks(self._h, _ptr(out), n.value, C.byref(n), C.byref(B), 1 if reset else 0))
        return out

    def set_anneal_block_records(self, records) -> None:
        rec = np.ascontiguousarray(records, dtype=np.uint64)
        if rec.ndim != 3 or rec.shape[1] != 2:
            raise AmcError(f"set_anneal_block_records: records of shape (n, 2, B), got {rec.shape}")
        _check(self._lib.amc_set_anneal_block_records(self._h, _ptr(rec), int(rec.shape[0]), int(rec.shape[2])))

    def anneal_block_counts(self) -> np.ndarray:
        """n_b, the chains of every block of families as they stand (synchronises)."""
        n, B = C.c_int(0), C.c_int(0)
        _check(self._lib.amc_anneal_fetch_blocks(self._h, None, 0, C.byref(n), C.byref(B), 0))
        out = np.zeros(B.value, dtype=np.uint64)
        _check(self._lib.amc_anneal_block_counts(self._h, _ptr(out)))
        return out

    # -- replica exchange along a temperature ladder (include/amc.h) ----------------
    def set_ladder(self, n_rungs: int) -> None:
        """Ladders of ``n_rungs`` consecutive global chain ids (0: none).  Needs a per-chain beta array and a shard made of whole
        ladders; zeroes the gap counters."""
        _check(self._lib.amc_set_ladder(self._h, int(n_rungs)))
        self.n_rungs = int(n_rungs)

    def exchange(self, n_steps: int = 1) -> None:
        """n exchange steps (asynchronous); the parity of the gaps alternates with the exchange step index."""
        _check(self._lib.amc_exchange(self._h, int(n_steps)))

    def sweep_exchange(self, n_rounds: int, sweeps_per_round: int = 1) -> None:
        """n_rounds x [sweep(sweeps_per_round); exchange(1)] queued by one call."""
        _check(self._lib.amc_sweep_exchange(self._h, int(n_rounds), int(sweeps_per_round)))

    def exchange_counters(self):
        """(accepted, attempted), one entry per gap r < R - 1: exact counts over this shard's ladders."""
        return self._i64_pair(self._lib.amc_exchange_counters, max(self.n_rungs - 1, 1))

    def set_exchange_counters(self, accepted, attempted) -> None:
        n = max(self.n_rungs - 1, 1)
        acc = np.ascontiguousarray(accepted, dtype=np.int64).reshape(-1)
        att = np.ascontiguousarray(attempted, dtype=np.int64).reshape(-1)
        if acc.size != n or att.size != n:
            raise AmcError(f"set_exchange_counters: one entry per gap ({n}) each")
        _check(self._lib.amc_set_exchange_counters(self._h, _ptr(acc), _ptr(att)))

    def histogram_rungs(self, lo: float, hi: float, n_bins: int) -> np.ndarray:
        """counts[R][n_bins + 3]: histogram() by rung (this shard only)."""
        n = self._rungs()
        out = np.zeros((n, int(n_bins) + 3), dtype=np.uint64)
        _check(self._lib.amc_histogram_rungs(self._h, float(lo), float(hi), int(n_bins), _ptr(out)))
        return out

    def reduce_rungs(self, columns: int = AMC_REDUCE_ALL) -> np.ndarray:
        """records[R][3][AMC_XSUM_WORDS]: per rung the reproducible sums of e, x, x^2 over this shard's ladders, one chain per summand
        (amc_reduce_rungs_exact); ``columns``: AMC_REDUCE_* bits, a column not asked for is an all-zero record.  What shards exchange
        (sharding.allreduce_xsum); ``xsum_round`` yields the Float64s.  Observes the state behind everything queued; synchronises."""
        n = self._rungs()
        out = np.zeros((n, 3, AMC_XSUM_WORDS), dtype=np.float64)
        _check(self._lib.amc_reduce_rungs_exact(self._h, int(columns), _ptr(out)))
        return out

    # -- bridge sums (include/amc.h; DESIGN.md section 3.13 "Bridge sums") ----------------
    def bridge_accumulate(self, columns: int = AMC_BRIDGE_ALL) -> None:
        """Queue one snapshot of the bridge sums -- per rung the reproducible sums of e, e^2 and the neighbour-reweighting factors
        WF, WB, MF = min(1, WF), MB = min(1, WB) -- into the device-resident accumulator (amc_bridge_accumulate).  Stream-ordered,
        nothing synchronises.  ``columns``: AMC_BRIDGE_* bits, fixed by the first call after a reset."""
        _check(self._lib.amc_bridge_accumulate(self._h, int(columns)))

    def bridge_fetch(self, reset: bool = False):
        """(records[R][6][AMC_XSUM_WORDS], n_snapshots) of this shard's accumulator, columns in the order E, EE, WF, WB, MF, MB
        (amc_bridge_fetch); ``reset`` zeroes both and frees the mask.  What shards exchange (sharding.allreduce_xsum); ``xsum_round``
        yields the Float64s.  Synchronises."""
        n = self._rungs()
        out = np.zeros((n, 6, AMC_XSUM_WORDS), dtype=np.float64)
        count = C.c_uint64(0)
        _check(self._lib.amc_bridge_fetch(self._h, _ptr(out), C.byref(count), int(bool(reset))))
        return out, int(count.value)

    def set_bridge(self, records=None, n_snapshots: int = 0) -> None:
        """Restore the accumulator from ``bridge_fetch``'s records and count (amc_set_bridge); ``None`` clears it.  The mask is read off
        the records: a column is in it exactly when its records are not all zero."""
        if records is None:
            _check(self._lib.amc_set_bridge(self._h, None, 0))
            return
        n = self._rungs()
        rec = np.ascontiguousarray(records, dtype=np.float64)
        if rec.size != n * 6 * AMC_XSUM_WORDS:
            raise AmcError(f"set_bridge: {rec.size} doubles, the records of {n} rungs take {n * 6 * AMC_XSUM_WORDS}")
        if int(n_snapshots) < 0:
            raise AmcError("set_bridge: n_snapshots < 0")
        _check(self._lib.amc_set_bridge(self._h, _ptr(rec), int(n_snapshots)))

    # -- time correlation (include/amc.h) ----------------
    def corr_mark(self, observable="energy") -> None:
        """Mark a time origin (amc_corr_mark): a_i = O(x_i) of every local chain is kept on the device, and sample 0 is taken in the
        same launch.  ``observable``: "energy" / "x" or AMC_CORR_E / AMC_CORR_X.  Stream-ordered, nothing synchronises."""
        _check(self._lib.amc_corr_mark(self._h, int(CORR_OBSERVABLES.get(observable, observable))))

    def corr_sample(self) -> None:
        """Queue the sums of O, O^2 and a O by group into the next slot of the mark (amc_corr_sample).  Stream-ordered."""
        _check(self._lib.amc_corr_sample(self._h))

    def corr_fetch(self):
        """(records[n_samples][G][3][AMC_XSUM_WORDS], steps[n_samples], observable) of this shard's mark, columns O, OO, AO
        (amc_corr_fetch); G = R with a ladder, else 1; observable 0 and no samples when nothing is marked.  What shards exchange
        (sharding.allreduce_xsum); ``xsum_round`` yields the Float64s.  Synchronises, resets nothing."""
        g = self._rungs()
        out = np.zeros((AMC_CORR_MAX_LAGS, g, AMC_CORR_COLS, AMC_XSUM_WORDS), dtype=np.float64)
        steps = np.zeros(AMC_CORR_MAX_LAGS, dtype=np.uint64)
        n, obs = C.c_int(0), C.c_int(0)
        _check(self._lib.amc_corr_fetch(self._h, _ptr(out), _ptr(steps), AMC_CORR_MAX_LAGS, C.byref(n), C.byref(obs)))
        return out[:n.value].copy(), steps[:n.value].copy(), int(obs.value)

    def corr_origin(self) -> np.ndarray:
        """a_i of every local chain as the mark stored it (amc_corr_download_origin; checkpoints).  Synchronises."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        _check(self._lib.amc_corr_download_origin(self._h, _ptr(out)))
        return out

    def set_corr(self, observable, origin, records, steps) -> None:
        """Restore a mark with its samples from ``corr_origin`` and ``corr_fetch`` (amc_set_corr; checkpoints)."""
        g = self._rungs()
        st = np.ascontiguousarray(steps, dtype=np.uint64)
        rec = np.ascontiguousarray(records, dtype=np.float64)
        org = np.ascontiguousarray(origin, dtype=np.float64)
        if org.size != self.n_chains or rec.size != st.size * g * AMC_CORR_COLS * AMC_XSUM_WORDS:
            raise AmcError(f"set_corr: {org.size} origin values and {rec.size} doubles for {st.size} samples of {g} groups on {self.n_chains} chains")
        _check(self._lib.amc_set_corr(self._h, int(CORR_OBSERVABLES.get(observable, observable)), _ptr(org), _ptr(rec), _ptr(st),
                                      int(st.size)))

    def corr_clear(self) -> None:
        """Drop the mark (amc_corr_clear); the memory stays."""
        _check(self._lib.amc_corr_clear(self._h))

    # -- convergence per group (include/amc.h) ----------------
    # (Not offered on a SplitEngine, as corr_mark is not.)
    def chain_stats_accumulate(self, observable="energy", part: int = 0) -> None:
        """Queue one sample of the observable into every local chain's running sums S and Q of ``part`` (0 or 1: the halves of the
        window; amc_chain_stats_accumulate).  ``observable``: "energy" / "x" or AMC_CORR_E / AMC_CORR_X, fixed by the first call
        after a clear.  Stream-ordered, nothing synchronises."""
        _check(self._lib.amc_chain_stats_accumulate(self._h, int(CORR_OBSERVABLES.get(observable, observable)), int(part)))

    def chain_stats_counts(self):
        """((n0, n1), observable): the samples each part holds and the observable the sums were begun with, 0 when nothing is
        accumulated (amc_chain_stats_fetch without records).  Host state: nothing is queued, nothing waits."""
        n = np.zeros(2, dtype=np.uint64)
        g, obs = C.c_int(0), C.c_int(0)
        _check(self._lib.amc_chain_stats_fetch(self._h, None, 0, _ptr(n), C.byref(g), C.byref(obs)))
        return (int(n[0]), int(n[1])), int(obs.value)

    def chain_stats_fetch(self):
        """(records[G][7][AMC_XSUM_WORDS], n[2], observable) of this shard: the sums over the chains of a group of S0, S0 S0, Q0, S1,
        S1 S1, Q1, S0 S1 and the samples each part holds (amc_chain_stats_fetch); G = R with a ladder, else 1; records of shape
        (G, 0, AMC_XSUM_WORDS), n = (0, 0) and observable 0 when nothing is accumulated.  What shards exchange
        (sharding.allreduce_xsum).  Synchronises, changes nothing."""
        n = np.zeros(2, dtype=np.uint64)
        g, obs = C.c_int(0), C.c_int(0)
        _check(self._lib.amc_chain_stats_fetch(self._h, None, 0, _ptr(n), C.byref(g), C.byref(obs)))      # the sizes alone: nothing waits
        if obs.value == 0:
            return np.zeros((g.value, 0, AMC_XSUM_WORDS)), (0, 0), 0
        out = np.zeros((g.value, AMC_CHAIN_STATS_COLS, AMC_XSUM_WORDS), dtype=np.float64)
        _check(self._lib.amc_chain_stats_fetch(self._h, _ptr(out), int(out.size), _ptr(n), C.byref(g), C.byref(obs)))
        return out, (int(n[0]), int(n[1])), int(obs.value)

    def chain_stats_sums(self) -> np.ndarray:
        """sums[2 parts][S, Q][n_chains] of every local chain (amc_chain_stats_download; checkpoints).  Synchronises."""
        out = np.zeros((AMC_CHAIN_STATS_PARTS, 2, self.n_chains), dtype=np.float64)
        _check(self._lib.amc_chain_stats_download(self._h, _ptr(out)))
        return out

    def set_chain_stats(self, observable=0, n=(0, 0), sums=None) -> None:
        """Restore the running sums from ``chain_stats_sums`` and ``chain_stats_fetch``'s n (amc_set_chain_stats; checkpoints);
        ``sums=None`` or n = (0, 0) clears."""
        cnt = np.ascontiguousarray(n, dtype=np.uint64)
        if cnt.size != AMC_CHAIN_STATS_PARTS:
            raise AmcError(f"set_chain_stats: n = {n!r} must hold the two counts")
        if sums is None or not cnt.any():
            _check(self._lib.amc_set_chain_stats(self._h, 0, None, None))
            return
        s = np.ascontiguousarray(sums, dtype=np.float64)
        if s.size != AMC_CHAIN_STATS_PARTS * 2 * self.n_chains:
            raise AmcError(f"set_chain_stats: {s.size} doubles, 2 parts of S and Q on {self.n_chains} chains take {4 * self.n_chains}")
        _check(self._lib.amc_set_chain_stats(self._h, int(CORR_OBSERVABLES.get(observable, observable)), _ptr(cnt), _ptr(s)))

    def chain_stats_clear(self) -> None:
        """Forget the running sums (amc_chain_stats_clear); the memory stays."""
        _check(self._lib.amc_chain_stats_clear(self._h))

    # -- energy histograms (include/amc.h) ----------------
    # (Not offered on a SplitEngine, as bridge_accumulate is not: the sub-shards of one GPU keep no ladder state.)
    def energy_histogram_accumulate(self, lo: float, hi: float, n_bins: int) -> None:
        """Queue one snapshot of the energy histograms -- per group (rung; one group without a ladder) the counts of
        e = potential(x) over ``n_bins`` half-open bins of [lo, hi) and the three cells below / at or above / NaN -- into the
        device-resident accumulator (amc_energy_histogram_accumulate).  Stream-ordered, nothing synchronises.  The bins are fixed by
        the first call after a reset."""
        _check(self._lib.amc_energy_histogram_accumulate(self._h, float(lo), float(hi), int(n_bins)))

    def energy_histogram_fetch(self, reset: bool = False):
        """(counts[G, n_bins + 3] uint64, n_snapshots, (lo, hi, n_bins)) of this shard's accumulator (amc_energy_histogram_fetch);
        counts add across shards.  With nothing accumulated: counts of shape (G, 0), 0 snapshots, (0.0, 0.0, 0).  ``reset`` frees
        the accumulator and its bins.  Synchronises."""
        ng, nb, lo, hi, count = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_uint64(0)
        sizes = (C.byref(ng), C.byref(nb), C.byref(lo), C.byref(hi), C.byref(count))
        _check(self._lib.amc_energy_histogram_fetch(self._h, None, 0, *sizes, 0))      # the sizes alone: nothing waits
        if nb.value == 0:
            return np.zeros((ng.value, 0), dtype=np.uint64), 0, (0.0, 0.0, 0)
        out = np.empty(ng.value * (nb.value + 3), dtype=np.uint64)
        _check(self._lib.amc_energy_histogram_fetch(self._h, _ptr(out), int(out.size), *sizes, int(bool(reset))))
        return out[:ng.value * (nb.value + 3)].reshape(ng.value, nb.value + 3).copy(), int(count.value), (lo.value, hi.value, nb.value)

    def set_energy_histogram(self, lo: float = 0.0, hi: float = 0.0, n_bins: int = 0, counts=None, n_snapshots: int = 0) -> None:
        """Restore the accumulator from ``energy_histogram_fetch``'s counts, count and bins (amc_set_energy_histogram; checkpoints);
        ``counts=None`` or ``n_snapshots=0`` clears it."""
        if counts is None or int(n_snapshots) == 0:
            _check(self._lib.amc_set_energy_histogram(self._h, 0.0, 0.0, 0, None, 0))
            return
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.size != self._rungs() * (int(n_bins) + 3):
            raise AmcError(f"set_energy_histogram: {c.size} counts, {self._rungs()} rows of {int(n_bins)} bins take {self._rungs() * (int(n_bins) + 3)}")
        if int(n_snapshots) < 0:
            raise AmcError("set_energy_histogram: n_snapshots < 0")
        _check(self._lib.amc_set_energy_histogram(self._h, float(lo), float(hi), int(n_bins), _ptr(c), int(n_snapshots)))

    # -- moments per energy bin (include/amc.h; DESIGN.md section 3.17 "Moments per bin") ----------------
    def energy_moments_accumulate(self, lo: float, hi: float, n_bins: int, mask: int, x_bound: float) -> None:
        """Queue one snapshot of the energy histograms WITH the sums of x, x^2 and [x > 0] per bin that ``mask`` selects
        (AMC_EMOM_X | AMC_EMOM_XX | AMC_EMOM_POS) into their own device-resident accumulator (amc_energy_moments_accumulate).
        Stream-ordered.  The form (bins, mask, ``x_bound``) is fixed by the first call after a reset."""
        _check(self._lib.amc_energy_moments_accumulate(self._h, float(lo), float(hi), int(n_bins), int(mask), float(x_bound)))

    def energy_moments_fetch(self, reset: bool = False):
        """(counts[G, n_bins + 4] uint64, sums[G, C, n_bins] int64, n_snapshots, (lo, hi, n_bins, mask, x_bound)) of this shard's
        accumulator (amc_energy_moments_fetch); both add across shards, and a sum cell times its quantum (``emom_quanta``) is the
        sum.  With nothing accumulated: shapes (G, 0) and (G, 0, 0), 0 snapshots, (0.0, 0.0, 0, 0, 0.0).  ``reset`` frees the
        accumulator and its form.  Synchronises."""
        ng, nb, nc, lo, hi = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        mask, bound, count = C.c_int(0), C.c_double(0.0), C.c_uint64(0)
        sizes = (C.byref(ng), C.byref(nb), C.byref(nc), C.byref(lo), C.byref(hi), C.byref(mask), C.byref(bound), C.byref(count))
        _check(self._lib.amc_energy_moments_fetch(self._h, None, None, 0, 0, *sizes, 0))      # the sizes alone: nothing waits
        if nb.value == 0:
            return np.zeros((ng.value, 0), dtype=np.uint64), np.zeros((ng.value, 0, 0), dtype=np.int64), 0, (0.0, 0.0, 0, 0, 0.0)
        counts = np.empty((ng.value, nb.value + 4), dtype=np.uint64)
        sums = np.empty((ng.value, nc.value, nb.value), dtype=np.int64)
        _check(self._lib.amc_energy_moments_fetch(self._h, _ptr(counts), _ptr(sums), int(counts.size), int(sums.size), *sizes, int(bool(reset))))
        return counts, sums, int(count.value), (lo.value, hi.value, nb.value, mask.value, bound.value)

    def set_energy_moments(self, lo: float = 0.0, hi: float = 0.0, n_bins: int = 0, mask: int = 0, x_bound: float = 0.0, counts=None, sums=None,
                           n_snapshots: int = 0) -> None:
        """Restore the accumulator from ``energy_moments_fetch``'s cells, count and form (amc_set_energy_moments; checkpoints);
        ``counts=None``, ``sums=None`` or ``n_snapshots=0`` clears it."""
        if counts is None or sums is None or int(n_snapshots) == 0:
            _check(self._lib.amc_set_energy_moments(self._h, 0.0, 0.0, 0, 0, 0.0, None, None, 0))
            return
        c, s = np.ascontiguousarray(counts, dtype=np.uint64), np.ascontiguousarray(sums, dtype=np.int64)
        G, cols = self._rungs(), bin(int(mask) & 0xFFFFFFFF).count("1")
        if c.size != G * (int(n_bins) + 4) or s.size != G * cols * int(n_bins):
            raise AmcError(f"set_energy_moments: {c.size} counts and {s.size} sums, {G} rows of {int(n_bins)} bins and {cols} columns take "
                           f"{G * (int(n_bins) + 4)} and {G * cols * int(n_bins)}")
        if int(n_snapshots) < 0:
            raise AmcError("set_energy_moments: n_snapshots < 0")
        _check(self._lib.amc_set_energy_moments(self._h, float(lo), float(hi), int(n_bins), int(mask), float(x_bound), _ptr(c), _ptr(s), int(n_snapshots)))

    # -- jackknife blocks (include/amc.h) ----------------
    def set_blocks(self, n_blocks: int, chunk: int = 0) -> None:
        """Keep the bridge sums and the time correlation per block of ladders, block of ladder l = (l_global div chunk) mod n_blocks
        (amc_set_blocks); ``n_blocks`` 0 turns the partition off, ``chunk`` 0 asks for the default.  Clears the bridge accumulator and
        the mark; energy histograms and moments per bin kept per block are folded into plain accumulators, nothing is lost.
        ``bridge_fetch`` / ``corr_fetch`` go on returning the merged records, bit for bit those of a handle without one."""
        _check(self._lib.amc_set_blocks(self._h, int(n_blocks), int(chunk)))

    def bridge_fetch_blocks(self, reset: bool = False):
        """(records[B][R][6][AMC_XSUM_WORDS], n_snapshots) of this shard's blocked accumulator (amc_bridge_fetch_blocks); a block
        without a local ladder is all zero.  Shards merge block by block (sharding.allreduce_xsum).  Synchronises."""
        out = np.zeros((AMC_MAX_JK_BLOCKS, self._rungs(), 6, AMC_XSUM_WORDS), dtype=np.float64)
        nb, count = C.c_int(0), C.c_uint64(0)
        _check(self._lib.amc_bridge_fetch_blocks(self._h, _ptr(out), AMC_MAX_JK_BLOCKS, C.byref(nb), C.byref(count), int(bool(reset))))
        return out[:nb.value].copy(), int(count.value)

    def corr_fetch_blocks(self):
        """(records[B][n_samples][G][3][AMC_XSUM_WORDS], steps[n_samples], observable) of this shard's blocked mark
        (amc_corr_fetch_blocks).  Synchronises, resets nothing."""
        nb, n, obs = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self._lib.amc_corr_fetch_blocks(self._h, None, None, 0, C.byref(nb), C.byref(n), C.byref(obs)))      # the sizes alone
        b, s = nb.value, n.value
        out = np.zeros((b, max(s, 1), self._rungs(), AMC_CORR_COLS, AMC_XSUM_WORDS), dtype=np.float64)
        steps = np.zeros(max(s, 1), dtype=np.uint64)
        _check(self._lib.amc_corr_fetch_blocks(self._h, _ptr(out), _ptr(steps), s, C.byref(nb), C.byref(n), C.byref(obs)))
        return out[:, :s].copy(), steps[:s].copy(), int(obs.value)

    def set_bridge_blocks(self, records=None, n_snapshots: int = 0) -> None:
        """Restore the blocked accumulator from ``bridge_fetch_blocks``'s records and count (amc_set_bridge_blocks; checkpoints);
        ``None`` clears it.  The partition is set beforehand."""
        if records is None:
            _check(self._lib.amc_set_bridge_blocks(self._h, None, 0, 0))
            return
        rec = np.ascontiguousarray(records, dtype=np.float64)
        per_block = self._rungs() * 6 * AMC_XSUM_WORDS
        if rec.ndim < 1 or rec.shape[0] < 1 or rec.size != rec.shape[0] * per_block:
            raise AmcError(f"set_bridge_blocks: {rec.size} doubles, the records of a block of {self._rungs()} rungs take {per_block}")
        if int(n_snapshots) < 0:
            raise AmcError("set_bridge_blocks: n_snapshots < 0")
        _check(self._lib.amc_set_bridge_blocks(self._h, _ptr(rec), int(rec.shape[0]), int(n_snapshots)))

    def set_corr_blocks(self, observable, origin, records, steps) -> None:
        """Restore a blocked mark with its samples from ``corr_origin`` and ``corr_fetch_blocks`` (amc_set_corr_blocks; checkpoints)."""
        g = self._rungs()
        st = np.ascontiguousarray(steps, dtype=np.uint64)
        rec = np.ascontiguousarray(records, dtype=np.float64)
        org = np.ascontiguousarray(origin, dtype=np.float64)
        if rec.ndim < 1 or rec.shape[0] < 1 or org.size != self.n_chains or rec.size != rec.shape[0] * st.size * g * AMC_CORR_COLS * AMC_XSUM_WORDS:
            raise AmcError(f"set_corr_blocks: {org.size} origin values and {rec.size} doubles for {st.size} samples of {g} groups on "
                           f"{self.n_chains} chains")
        _check(self._lib.amc_set_corr_blocks(self._h, int(CORR_OBSERVABLES.get(observable, observable)), _ptr(org), _ptr(rec), _ptr(st),
                                             int(rec.shape[0]), int(st.size)))

    # -- energy histograms per jackknife block (include/amc.h; DESIGN.md section 3.17 "Per block") ----------------
    def energy_histogram_accumulate_blocks(self, lo: float, hi: float, n_bins: int) -> None:
        """``energy_histogram_accumulate`` with a set of rows per block of the partition (amc_energy_histogram_accumulate_blocks):
        needs ``set_blocks``; the first call after a reset fixes the bins and the accumulator's form and waits for the stream once."""
        _check(self._lib.amc_energy_histogram_accumulate_blocks(self._h, float(lo), float(hi), int(n_bins)))

    def energy_histogram_fetch_blocks(self, reset: bool = False):
        """(counts[B, G, n_bins + 3] uint64, n_snapshots, (lo, hi, n_bins)) of this shard's blocked accumulator
        (amc_energy_histogram_fetch_blocks); a block without a local ladder is all zero, shards add cell by cell.  An AmcError unless
        a blocked accumulator stands.  ``reset`` frees the accumulator.  Synchronises."""
        nk, ng, nb, lo, hi, count = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_uint64(0)
        sizes = (C.byref(nk), C.byref(ng), C.byref(nb), C.byref(lo), C.byref(hi), C.byref(count))
        _check(self._lib.amc_energy_histogram_fetch_blocks(self._h, None, 0, *sizes, 0))      # the sizes alone: nothing waits
        shape = (nk.value, ng.value, nb.value + 3)
        out = np.empty(shape[0] * shape[1] * shape[2], dtype=np.uint64)
        _check(self._lib.amc_energy_histogram_fetch_blocks(self._h, _ptr(out), int(out.size), *sizes, int(bool(reset))))
        return out.reshape(shape), int(count.value), (lo.value, hi.value, nb.value)

    def set_energy_histogram_blocks(self, lo: float = 0.0, hi: float = 0.0, n_bins: int = 0, counts=None, n_snapshots: int = 0) -> None:
        """Restore the blocked accumulator from ``energy_histogram_fetch_blocks``'s counts, count and bins
        (amc_set_energy_histogram_blocks; checkpoints); ``counts=None`` or ``n_snapshots=0`` clears it.  The partition is set
        beforehand."""
        if counts is None or int(n_snapshots) == 0:
            _check(self._lib.amc_set_energy_histogram_blocks(self._h, 0.0, 0.0, 0, None, 0, 0))
            return
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        per_block = self._rungs() * (int(n_bins) + 3)
        if c.ndim < 1 or c.shape[0] < 1 or c.size != c.shape[0] * per_block:
            raise AmcError(f"set_energy_histogram_blocks: {c.size} counts, a block of {self._rungs()} rows of {int(n_bins)} bins takes {per_block}")
        if int(n_snapshots) < 0:
            raise AmcError("set_energy_histogram_blocks: n_snapshots < 0")
        _check(self._lib.amc_set_energy_histogram_blocks(self._h, float(lo), float(hi), int(n_bins), _ptr(c), int(c.shape[0]), int(n_snapshots)))

    # -- moments per energy bin per jackknife block (include/amc.h; DESIGN.md section 3.17 "Moments per block") ----------------
    def energy_moments_accumulate_blocks(self, lo: float, hi: float, n_bins: int, mask: int, x_bound: float) -> None:
        """``energy_moments_accumulate`` with a set of cells per block of the partition (amc_energy_moments_accumulate_blocks): needs
        ``set_blocks``; the first call after a reset fixes the form and waits for the stream once."""
        _check(self._lib.amc_energy_moments_accumulate_blocks(self._h, float(lo), float(hi), int(n_bins), int(mask), float(x_bound)))

    def energy_moments_fetch_blocks(self, reset: bool = False):
        """(counts[B, G, n_bins + 4] uint64, sums[B, G, C, n_bins] int64, n_snapshots, (lo, hi, n_bins, mask, x_bound)) of this shard's
        blocked accumulator (amc_energy_moments_fetch_blocks); a block without a local ladder is all zero, shards add cell by cell.
        An AmcError unless a blocked accumulator stands.  ``reset`` frees the accumulator.  Synchronises."""
        nk, ng, nb, nc, lo, hi = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        mask, bound, count = C.c_int(0), C.c_double(0.0), C.c_uint64(0)
        sizes = (C.byref(nk), C.byref(ng), C.byref(nb), C.byref(nc), C.byref(lo), C.byref(hi), C.byref(mask), C.byref(bound), C.byref(count))
        _check(self._lib.amc_energy_moments_fetch_blocks(self._h, None, None, 0, 0, *sizes, 0))      # the sizes alone: nothing waits
        counts = np.empty((nk.value, ng.value, nb.value + 4), dtype=np.uint64)
        sums = np.empty((nk.value, ng.value, nc.value, nb.value), dtype=np.int64)
        _check(self._lib.amc_energy_moments_fetch_blocks(self._h, _ptr(counts), _ptr(sums), int(counts.size), int(sums.size), *sizes, int(bool(reset))))
        return counts, sums, int(count.value), (lo.value, hi.value, nb.value, mask.value, bound.value)

    def set_energy_moments_blocks(self, lo: float = 0.0, hi: float = 0.0, n_bins: int = 0, mask: int = 0, x_bound: float = 0.0, counts=None,
                                  sums=None, n_snapshots: int = 0) -> None:
        """Restore the blocked accumulator from ``energy_moments_fetch_blocks``'s cells, count and form (amc_set_energy_moments_blocks;
        checkpoints); ``counts=None``, ``sums=None`` or ``n_snapshots=0`` clears it.  The partition is set beforehand."""
        if counts is None or sums is None or int(n_snapshots) == 0:
            _check(self._lib.amc_set_energy_moments_blocks(self._h, 0.0, 0.0, 0, 0, 0.0, None, None, 0, 0))
            return
        c, s = np.ascontiguousarray(counts, dtype=np.uint64), np.ascontiguousarray(sums, dtype=np.int64)
        G, cols = self._rungs(), bin(int(mask) & 0xFFFFFFFF).count("1")
        per_c, per_s = G * (int(n_bins) + 4), G * cols * int(n_bins)
        if c.ndim < 1 or c.shape[0] < 1 or s.ndim < 1 or s.shape[0] != c.shape[0] or c.size != c.shape[0] * per_c or s.size != c.shape[0] * per_s:
            raise AmcError(f"set_energy_moments_blocks: {c.size} counts and {s.size} sums, a block of {G} rows of {int(n_bins)} bins and {cols} "
                           f"columns takes {per_c} and {per_s}")
        if int(n_snapshots) < 0:
            raise AmcError("set_energy_moments_blocks: n_snapshots < 0")
        _check(self._lib.amc_set_energy_moments_blocks(self._h, float(lo), float(hi), int(n_bins), int(mask), float(x_bound), _ptr(c), _ptr(s),
                                                       int(c.shape[0]), int(n_snapshots)))

    # -- walker tracking (include/amc.h; DESIGN.md section 3.13 "Walker tracking") ----------------
    def set_tracking(self, on: bool = True) -> None:
        """Turn walker tracking on (needs a ladder; labels start as the identity, the trip counters at zero) or off (frees the labels)."""
        _check(self._lib.amc_set_tracking(self._h, 1 if on else 0))

    def labels(self):
        """(walker, direction), two uint8 arrays with one entry per local chain: the walker id in [0, R) and the end the replica last
        visited (0 none yet, 1 rung 0, 2 rung R - 1).  Synchronises."""
        lab = np.zeros(self.n_chains, dtype=np.uint8)
        _check(self._lib.amc_download_labels(self._h, _ptr(lab)))
        return lab & np.uint8(63), lab >> np.uint8(6)

    def set_labels(self, walker, direction) -> None:
        w = np.ascontiguousarray(walker, dtype=np.int64).reshape(-1)
        d = np.ascontiguousarray(direction, dtype=np.int64).reshape(-1)
        if w.size != self.n_chains or d.size != self.n_chains:
            raise AmcError(f"set_labels: one walker id and one direction per local chain ({self.n_chains}) each")
        if w.size and (w.min() < 0 or w.max() > 63 or d.min() < 0 or d.max() > 3):
            raise AmcError("set_labels: walker ids must lie in [0, 64) and directions in [0, 4)")
        lab = np.ascontiguousarray(w | (d << 6), dtype=np.uint8)
        _check(self._lib.amc_upload_labels(self._h, _ptr(lab)))

    def flow_rungs(self) -> np.ndarray:
        """counts[R][3]: the local chains at rung r whose label has direction d (this shard only), int64."""
        n = self._rungs()
        out = np.zeros((n, 3), dtype=np.uint64)
        _check(self._lib.amc_flow_rungs(self._h, _ptr(out)))
        return out.astype(np.int64)

    def tracking_counters(self):
        """(round_trips, up_trips) over this shard's ladders since tracking was turned on: exact counts."""
        rt, up = C.c_int64(0), C.c_int64(0)
        _check(self._lib.amc_tracking_counters(self._h, C.byref(rt), C.byref(up)))
        return rt.value, up.value

    def set_tracking_counters(self, round_trips: int, up_trips: int) -> None:
        _check(self._lib.amc_set_tracking_counters(self._h, int(round_trips), int(up_trips)))

    # -- proposal widths per rung (include/amc.h; DESIGN.md section 3.13 "Widths per rung") ----------------
    def set_rung_sigma(self, sigma) -> None:
        """``sigma[K][R]``: the width of move k for the chains at rung r (needs a ladder and per-chain counters); ``None`` clears the
        table.  Stream-ordered; the sweeps that follow step every chain with the widths of its rung."""
        if sigma is None:
            _check(self._lib.amc_set_rung_sigma(self._h, None, 0))
            return
        s = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
        _check(self._lib.amc_set_rung_sigma(self._h, _ptr(s), int(s.size)))

    def rung_sigma(self) -> np.ndarray:
        """The table in force, shape (K, R): as it was set, or -- once a tuning has been queued -- as the device holds it (the host
        then waits for the queued steps)."""
        n = self._rungs()
        out = np.zeros((self.n_moves, n), dtype=np.float64)
        _check(self._lib.amc_get_rung_sigma(self._h, _ptr(out), int(out.size)))
        return out

    # -- respacing the ladder (include/amc.h; DESIGN.md section 3.13 "Respacing") ----------------
    def respace_ladder(self, rule, gamma: float = 1.0, eps: float = 0.0, counts=None) -> None:
        """Queue one respacing of the ladder: ``rule`` "acceptance" (equalise the rejection rate per gap) or "flow" (the
        feedback-optimised ladder; needs tracking when ``counts`` is None).  ``counts`` None: this handle's own counters, right only
        when it holds every ladder -- nothing synchronises.  Otherwise the GLOBAL counts: for "acceptance" attempted[R - 1] then
        accepted[R - 1], for "flow" n[R][3] as ``flow_rungs`` gives them.  ``respace_status`` tells what became of it."""
        rule_id = RESPACE_RULES.get(rule, rule)
        if not isinstance(rule_id, (int, np.integer)):
            raise AmcError(f"respace_ladder: rule {rule!r} is none of {sorted(RESPACE_RULES)}")
        ptr = None
        if counts is not None:
            R = self.n_rungs
            c = np.ascontiguousarray(counts).reshape(-1)
            if c.size and (not np.all(np.isfinite(c)) or c.min() < 0 or np.any(c != np.floor(c))):
                raise AmcError("respace_ladder: counts must be non-negative integers")
            c = np.ascontiguousarray(c, dtype=np.uint64)
            need = 2 * (R - 1) if rule_id == AMC_RESPACE_ACCEPTANCE else 3 * R
            if c.size != need:
                raise AmcError(f"respace_ladder: counts has {c.size} entries, rule {rule!r} with {R} rungs takes {need}")
            ptr = _ptr(c)
        _check(self._lib.amc_respace_ladder(self._h, int(rule_id), float(gamma), float(eps), ptr))

    def respace_status(self):
        """(status of the last respacing, number of status-0 respacings since the ladder was set).  Synchronises."""
        st, n = C.c_int(0), C.c_int64(0)
        _check(self._lib.amc_respace_status(self._h, C.byref(st), C.byref(n)))
        return st.value, n.value

    def set_respaced(self, n_respaced: int) -> None:
        _check(self._lib.amc_set_respaced(self._h, int(n_respaced)))

    def ladder(self) -> np.ndarray:
        """The R beta values of the ladder as the device holds them (the first local ladder).  Synchronises."""
        out = np.zeros(self._rungs(), dtype=np.float64)
        _check(self._lib.amc_get_ladder(self._h, _ptr(out)))
        return out

    # -- tuning the widths per rung (include/amc.h; DESIGN.md section 3.13 "Tuning the widths") ----------------
    def _cells(self):
        return self.n_moves, self._rungs()             # the shape (K, R) of a table per (move, rung)

    def tune_rung_sigma(self, target: float = 0.44, gamma: float = 1.0, min_calls: int = 1000, sigma_lo: float = 1e-100,
                        sigma_hi: float = 1e100, counts=None) -> None:
        """Queue one tuning of the table: every entry takes the damped step sigma <- sigma a / target with the acceptance a of its
        window.  ``counts`` None: this handle's own window, right only when it holds every ladder -- nothing synchronises.  Otherwise
        the GLOBAL window, (accepted, total), each of shape (K, R).  ``tune_status`` tells what became of every entry."""
        ptr = None
        if counts is not None:
            K, R = self._cells()
            try:
                c = np.ascontiguousarray(np.concatenate([np.asarray(counts[0]).reshape(-1), np.asarray(counts[1]).reshape(-1)]))
            except Exception as exc:
                raise AmcError(f"tune_rung_sigma: counts must be (accepted, total), each of shape ({K}, {R}) ({exc})") from None
            if c.size != 2 * K * R:
                raise AmcError(f"tune_rung_sigma: counts has {c.size} entries, the table of {K} moves x {R} rungs takes 2 x {K * R}")
            if c.dtype.kind not in "iu" and (not np.all(np.isfinite(c)) or np.any(c != np.floor(c))):
                raise AmcError("tune_rung_sigma: counts must be integers")
            c = np.ascontiguousarray(c, dtype=np.int64)
            ptr = _ptr(c)
        _check(self._lib.amc_tune_rung_sigma(self._h, float(target), float(gamma), int(min_calls), float(sigma_lo), float(sigma_hi), ptr))

    def tune_status(self):
        """(status per entry of the last tuning, shape (K, R); number of calls that tuned at least one entry since the table was set).
        Synchronises."""
        K, R = self._cells()
        st = np.zeros((K, R), dtype=np.int32)
        n = C.c_int64(0)
        _check(self._lib.amc_tune_status(self._h, _ptr(st), int(st.size), C.byref(n)))
        return st, n.value

    def set_tuned(self, n_tuned: int) -> None:
        _check(self._lib.amc_set_tuned(self._h, int(n_tuned)))

    def rung_window_counts(self):
        """(accepted, total) of this shard over the current window, each of shape (K, R); -1 in both where the counters were replaced
        behind the window's start.  Synchronises, changes nothing."""
        return self._i64_pair(self._lib.amc_rung_window_counts, self._cells())

    def rung_window_restart(self) -> None:
        """The window starts here (stream-ordered, nothing is read back)."""
        _check(self._lib.amc_rung_window_restart(self._h))

    def rung_window_base(self):
        """(accepted, total) per (move, rung) as they stood when the window began."""
        return self._i64_pair(self._lib.amc_rung_window_base, self._cells())

    def set_rung_window_base(self, accepted, total) -> None:
        K, R = self._cells()
        a = np.ascontiguousarray(accepted, dtype=np.int64).reshape(-1)
        t = np.ascontiguousarray(total, dtype=np.int64).reshape(-1)
        if a.size != K * R or t.size != K * R:
            raise AmcError(f"set_rung_window_base: {a.size} and {t.size} entries, the window of {K} moves x {R} rungs has {K * R}")
        _check(self._lib.amc_set_rung_window_base(self._h, _ptr(a), _ptr(t)))

    def rung_counter_totals(self):
        """(accepted, total), each of shape (K, R): the Move counters summed over this shard's ladders per (move, rung), exact."""
        return self._i64_pair(self._lib.amc_rung_counter_totals, self._cells())

    def sync(self) -> None:
        _check(self._lib.amc_sync(self._h))

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        _check(self._lib.amc_get_stream(self._h, C.byref(s)))
        return s.value or 0

    def timing_begin(self) -> None:
        _check(self._lib.amc_timing_begin(self._h))

    def timing_end(self) -> float:
        ms = C.c_double(0.0)
        _check(self._lib.amc_timing_end(self._h, C.byref(ms)))
        return ms.value

    def timing_mark(self) -> None:
        """Record the end event now (asynchronous); timing_end then waits for it and returns the elapsed device time."""
        _check(self._lib.amc_timing_mark(self._h))

    # -- RCCL through the C ABI (what the Julia binding uses) ----------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(load().amc_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank: int, n_ranks: int, unique_id: bytes) -> None:
        buf = C.create_string_buffer(unique_id, 128)
        _check(self._lib.amc_comm_init(self._h, int(rank), int(n_ranks), buf))

    def allreduce_sum(self, a: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        _check(self._lib.amc_allreduce_sum(self._h, _ptr(a), int(a.size)))
        return a

    def allreduce_xsum(self, records: np.ndarray) -> np.ndarray:
        """The merged records of all shards (amc_allreduce_xsum: one RCCL all-reduce used as a gather, then the integer merge)."""
        a = np.ascontiguousarray(records, dtype=np.float64).copy()
        _check(self._lib.amc_allreduce_xsum(self._h, _ptr(a), int(a.size // AMC_XSUM_WORDS)))
        return a

    def comm_destroy(self) -> None:
        """Drop the communicator: a single shard again."""
        _check(self._lib.amc_comm_destroy(self._h))

    def comm_info(self) -> dict:
        """What RCCL reports about this engine's communicator: ranks it spans, this rank, RCCL version, the librccl file."""
        n, r, v = C.c_int(0), C.c_int(0), C.c_int(0)
        path = C.create_string_buffer(1024)
        _check(self._lib.amc_comm_info(self._h, C.byref(n), C.byref(r), C.byref(v), path, 1024))
        return {"n_ranks": n.value, "rank": r.value, "rccl_version": v.value, "librccl": path.value.decode()}


class SplitEngine:
    """The shard of one GPU as `n_parts` sub-shards, each a HipEngine with its own stream.

    A single-sweep launch spends ~3 us in its launch boundary and ~2 us waiting for far memory at its ends; sub-shards
    on separate streams overlap one's ends with the other's body (31.3 -> 28.7 us per sweep of 1e7 chains measured with
    two).  Chains keep their GLOBAL ids, so every per-chain result is identical to the unsplit engine's; sums
    (reductions, gradient data) are merged over the parts on the host as exact integer records (reproducible sums), i.e. they
    are bit-identical to the unsplit engine's too.
    The device-resident estimator / update path (pg_accumulate, pg_update, pgmc_steps) is not offered: those keep
    per-engine state; PolicyGradientEstimator falls back to the host path (pg_estimate) on a split engine."""

    def __init__(self, *, n_chains: int, chain_offset: int = 0, n_chains_global: Optional[int] = None, n_parts: int = 2,
                 **kw):
        if chain_offset % 2:
            raise AmcError("chain_offset must be even")
        self.n_chains = int(n_chains)
        n_glob = int(n_chains_global if n_chains_global is not None else chain_offset + n_chains)
        n_pairs = (self.n_chains + 1) // 2
        n_parts = max(1, min(int(n_parts), n_pairs))
        bounds = [min(2 * ((i * n_pairs) // n_parts), self.n_chains) for i in range(n_parts)] + [self.n_chains]
        self.bounds = bounds
        self.parts = [HipEngine(n_chains=bounds[i + 1] - bounds[i], chain_offset=chain_offset + bounds[i],
                                n_chains_global=n_glob, **kw) for i in range(n_parts)]
        self.n_moves = self.parts[0].n_moves

    def close(self) -> None:
        for p in self.parts:
            p.close()

    def _slices(self):
        return [slice(self.bounds[i], self.bounds[i + 1]) for i in range(len(self.parts))]

    def upload_state(self, x, beta=None) -> None:
        x = np.ascontiguousarray(x, dtype=np.float64)
        for p, sl in zip(self.parts, self._slices()):
            p.upload_state(x[sl], None if beta is None else np.ascontiguousarray(beta, dtype=np.float64)[sl])

    def init_uniform(self, lo, hi) -> None:
        for p in self.parts:
            p.init_uniform(lo, hi)

    def download_state(self, want_e: bool = True):
        xs, es = zip(*[p.download_state(want_e) for p in self.parts])
        return np.concatenate(xs), (np.concatenate(es) if want_e else None)

    def download_counters(self):
        a, t = zip(*[p.download_counters() for p in self.parts])
        return np.concatenate(a, axis=1), np.concatenate(t, axis=1)

    def counter_totals(self):
        a, t = zip(*[p.counter_totals() for p in self.parts])
        return np.sum(a, axis=0), np.sum(t, axis=0)

    def upload_counters(self, accepted, total=None) -> None:
        a = np.ascontiguousarray(accepted, dtype=np.int64).reshape(self.n_moves, self.n_chains)
        t = None if total is None else np.ascontiguousarray(total, dtype=np.int64).reshape(self.n_moves, self.n_chains)
        for p, sl in zip(self.parts, self._slices()):
            p.upload_counters(a[:, sl], None if t is None else t[:, sl])

    def set_counter_totals(self, accepted: int, steps_counted: int) -> None:
        for i, p in enumerate(self.parts):          # the pool-wide total lives in the first part, the step count in all
            p.set_counter_totals(int(accepted) if i == 0 else 0, steps_counted)

    def histogram(self, lo, hi, n_bins):
        return np.sum([p.histogram(lo, hi, n_bins) for p in self.parts], axis=0).astype(np.uint64)

    def download_strided(self, first: int, stride: int, count: int) -> np.ndarray:
        idx = int(first) + int(stride) * np.arange(int(count), dtype=np.int64)
        out = np.empty(int(count), dtype=np.float64)
        for p, sl in zip(self.parts, self._slices()):
            sel = np.nonzero((idx >= sl.start) & (idx < sl.stop))[0]
            if sel.size:
                out[sel] = p.download_strided(int(idx[sel[0]] - sl.start), int(stride), int(sel.size))
        return out

    def sweep(self, n_sweeps: int = 1) -> None:
        for p in self.parts:          # asynchronous: the parts' launches overlap
            p.sweep(n_sweeps)

    @property
    def step(self) -> int:
        return self.parts[0].step

    @step.setter
    def step(self, t: int) -> None:
        for p in self.parts:
            p.step = t

    @property
    def estimator_step(self) -> int:
        return self.parts[0].estimator_step

    @estimator_step.setter
    def estimator_step(self, t: int) -> None:
        for p in self.parts:
            p.estimator_step = t

    def reduce(self) -> np.ndarray:
        rec, steps = self.reduce_exact()
        return self.parts[0].reduce_records_value(rec, steps)

    def reduce_exact(self):
        self.reduce_begin()
        return self.reduce_end_exact()

    def reduce_end_exact(self):
        rec, steps = None, 0
        for p in self.parts:          # integer merges: the split does not enter the result
            r, steps = p.reduce_end_exact()
            rec = r if rec is None else xsum_merge(rec, r)
        return rec, steps

    def reduce_records_value(self, records, steps_counted):
        return self.parts[0].reduce_records_value(records, steps_counted)

    @property
    def per_chain_counters(self) -> bool:
        return self.parts[0].per_chain_counters

    def reduce_begin(self) -> None:
        for p in self.parts:
            p.reduce_begin()

    def sweep_reduce_begin(self, n_sweeps: int = 1) -> None:
        for p in self.parts:
            p.sweep_reduce_begin(n_sweeps)

    def reduce_end(self) -> np.ndarray:
        rec, steps = self.reduce_end_exact()
        return self.parts[0].reduce_records_value(rec, steps)

    def set_parameters(self, k, p_) -> None:
        for p in self.parts:
            p.set_parameters(k, p_)

    def get_parameters(self, k):
        return self.parts[0].get_parameters(k)

    def pg_estimate_exact(self, learn_ids, q_batch) -> np.ndarray:
        rec = None
        for p in self.parts:
            r = p.pg_estimate_exact(learn_ids, q_batch)
            rec = r if rec is None else xsum_merge(rec, r).reshape(r.shape)
        return rec

    def pg_estimate(self, learn_ids, q_batch) -> np.ndarray:
        rec = self.pg_estimate_exact(learn_ids, q_batch)
        return xsum_round(rec).reshape(rec.shape[0], rec.shape[1])

    def sync(self) -> None:
        for p in self.parts:
            p.sync()

    def timing_begin(self) -> None:
        self.sync()
        self._t0 = time.perf_counter()

    def timing_end(self) -> float:
        """Wall-clock ms between timing_begin and the completion of everything queued since (the parts run on
        different streams: there is no single pair of stream events that brackets them)."""
        self.sync()
        return (time.perf_counter() - self._t0) * 1e3


def selftest_math(fn: str, a: np.ndarray, b: Optional[np.ndarray] = None, device: int = 0) -> np.ndarray:
    """Evaluate one arithmetic-spec primitive on the GPU (parity tests only)."""
    ids = {"exp": 0, "log": 1, "sinpi": 2, "cospi": 3, "sqrt": 4, "div": 5, "div_by_const": 6, "logbm": 7,
           "sqrt_radius": 8, "log_proposal_density": 9, "grad_log_proposal_density": 10,
           "grad_log_proposal_density_kernel_form": 11}
    a = np.ascontiguousarray(a, dtype=np.float64)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    _check(load().amc_selftest_math(int(device), ids[fn], _ptr(a), _ptr(b), _ptr(out), a.size))
    return out


def selftest_accept_filter(t_from: float, t_to: float, device: int = 0) -> float:
    """Largest relative deviation of the accept filter's float estimate from the spec's f64 exp over EVERY float in
    [t_to, t_from] (t_to <= t_from <= 0), measured on the GPU (parity tests only)."""
    out = C.c_double(0.0)
    _check(load().amc_selftest_accept_filter(int(device), C.c_float(t_from), C.c_float(t_to), C.byref(out)))
    return out.value


def selftest_filter_argument(beta: float, sigma: float, x: np.ndarray, delta: np.ndarray, device: int = 0) -> np.ndarray:
    """y (Float32) of the K == 1 harmonic sweeps' filter argument for positions x and displacements delta, evaluated on the device."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    delta = np.ascontiguousarray(delta, dtype=np.float64)
    assert x.shape == delta.shape
    out = np.empty(x.shape, dtype=np.float32)
    _check(load().amc_selftest_filter_argument(int(device), C.c_double(beta), C.c_double(sigma), _ptr(x), _ptr(delta), _ptr(out), x.size))
    return out


def selftest_philox(seed: int, pair: np.ndarray, t: np.ndarray, draw: int, stream: int,
                    device: int = 0) -> np.ndarray:
    """Raw Philox4x32-10 words of draw (pair, t, draw, stream) on the GPU (parity tests only)."""
    pair = np.ascontiguousarray(pair, dtype=np.uint64)
    t = np.ascontiguousarray(t, dtype=np.uint64)
    out = np.empty((pair.size, 4), dtype=np.uint32)
    _check(load().amc_selftest_philox(int(device), C.c_uint64(int(seed)), _ptr(pair), _ptr(t), int(draw), int(stream), _ptr(out), pair.size))
    return out


def selftest_wave_totals(values: np.ndarray, device: int = 0):
    """The kernels' wave-wide integer totals of values[6][64] (int64) on the GPU: (totals[13], totals_plain[6]), see
    include/amc.h (parity tests only)."""
    values = np.ascontiguousarray(values, dtype=np.int64)
    assert values.shape == (6, 64)
    out = np.zeros(13, dtype=np.int64)
    ref = np.zeros(6, dtype=np.int64)
    _check(load().amc_selftest_wave_totals(int(device), _ptr(values), _ptr(out), _ptr(ref)))
    return out, ref


def selftest_staged_tables(device: int = 0) -> np.ndarray:
    """The 546 doubles of the math tables as a block holds them in LDS, staged and copied out on the GPU (parity tests only)."""
    out = np.empty(546, dtype=np.float64)
    _check(load().amc_selftest_staged_tables(int(device), _ptr(out)))
    return out
