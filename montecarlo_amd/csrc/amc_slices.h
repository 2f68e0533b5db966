// amc_slices.h -- the slice plan of the single-sweep launches (amc_sweeps.hip sweep_launches_sliced): an ensemble's pairs cut into
// up to AMC_MAX_SLICES contiguous slices, each the whole ensemble of a sweep_kernel launch of its own on a stream of its own.
// Pure host arithmetic: nothing here needs HIP (tests/test_slice_plan.py compiles it into a plain C++ program).
#pragma once

#include <cstdint>

namespace amc {

constexpr int AMC_MAX_SLICES = 3;      // with the engine's communication stream: four streams per handle at most

struct Slice {
    int64_t first_pair = 0;     // local pair the slice starts at: a multiple of `block`, so x + 2 * first_pair keeps load_pair_block's alignment
    int64_t n_chains = 0;       // chains of the slice: 2 * block * (its blocks), except the last slice, which ends where the ensemble ends
    int grid = 0;               // blocks of its launch: <= n_slots (the slices share the per-block accepted slots)
    int32_t full_rounds = 0;    // SweepArgs.full_rounds / tail_pairs of that grid: full_rounds * grid * block + tail_pairs == pairs of the slice
    int32_t tail_pairs = 0;
};

struct SlicePlan {
    int count = 0;              // slices that hold pairs (an ensemble of fewer blocks than slices: fewer; no chains: none)
    Slice s[AMC_MAX_SLICES];
};

// Whole blocks of `block` pairs are dealt out evenly, the first slices taking the remainder, so every boundary is a multiple of
// `block` pairs and only the last slice can be ragged or end in a lone chain.  A slice's launch reads nothing beyond its last
// block, and stores nothing beyond its last chain.
inline SlicePlan plan_slices(int64_t n_chains, int block, int slices, int n_cu, int blocks_per_cu, int n_slots)
{
    SlicePlan plan;
    if (n_chains <= 0 || block <= 0) return plan;
    if (slices < 1) slices = 1;
    if (slices > AMC_MAX_SLICES) slices = AMC_MAX_SLICES;
    const int64_t n_pairs = (n_chains + 1) / 2;
    const int64_t n_blocks = (n_pairs + block - 1) / block;
    const int64_t each = n_blocks / slices, extra = n_blocks % slices;
    int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 1) * (blocks_per_cu > 0 ? blocks_per_cu : 1);
    if (n_slots > 0 && cap > n_slots) cap = n_slots;
    int64_t first_block = 0;
    for (int i = 0; i < slices; ++i) {
        const int64_t blocks = each + (i < extra ? 1 : 0);
        if (blocks == 0) break;      // (the slices behind it are empty too)
        Slice& sl = plan.s[plan.count++];
        sl.first_pair = first_block * block;
        first_block += blocks;
        const bool last = first_block == n_blocks;
        const int64_t pairs = last ? n_pairs - sl.first_pair : blocks * block;
        sl.n_chains = last ? n_chains - 2 * sl.first_pair : 2 * pairs;
        sl.grid = (int)(blocks < cap ? blocks : cap);
        const int64_t round = (int64_t)sl.grid * block;
        sl.full_rounds = (int32_t)(pairs / round);
        sl.tail_pairs = (int32_t)(pairs % round);
    }
    return plan;
}

}  // namespace amc
