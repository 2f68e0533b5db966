// blocks_plan_host.cpp -- the traversal of the blocked passes (montecarlo_amd/csrc/amc_blocks.h: blk::walk_begin / walk_next, the launch
// split blk::ladders_per_launch, the closed-form counts blk::ladders_in_block) enumerated on the host: every (launch, HIP block, thread,
// trip) of a pass, as bridge_sums_blocks_kernel and corr_sums_blocks_kernel walk it.
//
//   blocks_plan_host            runs the whole matrix below and prints "ok <configurations>"; any violated property prints the
//                               configuration and exits with status 1
// Properties, per configuration (G, B, C, grid, ladders, first global ladder, lane cap):
//   every local ladder is visited exactly once, inside its launch's range, by a HIP block k with k mod B == b(ladder);
//   no lane takes more than `cap` ladders in one launch; a finished walk stays finished;
//   ladders_in_block(b) is the number of local ladders of block b.
// Build: c++ -std=c++17 with -fsanitize=address,undefined (tests/test_blocks_plan_host.py); with AMC_BLOCKS_INDEX_ONLY the header is
// plain host C++ once the two qualifiers are empty.
#define __host__
#define __device__
#define AMC_BLOCKS_INDEX_ONLY
#include "amc_blocks.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace blk = amc::blk;

static const int THREADS = 256;

static int check(int G, int B, int64_t C, int grid, int64_t n, int64_t first, int64_t cap)
{
    blk::Part part = {};
    part.l_first = first;
    part.chunk = C;
    part.n_blocks = B;
    auto bad = [&](const char* what, int64_t v) {
        std::printf("FAILED %s (%lld): G=%d B=%d C=%lld grid=%d ladders=%lld first=%lld cap=%lld\n", what, (long long)v, G, B, (long long)C, grid,
                    (long long)n, (long long)first, (long long)cap);
        return 1;
    };
    if (grid % B) return bad("grid is no multiple of B", grid);
    std::vector<unsigned char> seen((size_t)n, 0);
    std::vector<int64_t> in_block((size_t)B, 0);
    const int64_t per_launch = blk::ladders_per_launch(n, B, C, G, grid, THREADS, cap);
    if (per_launch < 1) return bad("per_launch", per_launch);
    for (int64_t l_begin = 0; l_begin < n; l_begin += per_launch) {
        const int64_t l_end = l_begin + per_launch < n ? l_begin + per_launch : n;
        for (int k = 0; k < grid; ++k) {
            for (int t = 0; t < THREADS; ++t) {
                blk::Walk w;
                const int g = blk::walk_begin(w, part, G, grid, THREADS, k, t, l_begin, l_end);
                if (t == 0 && w.q >= w.q_stop) break;              // the HIP block has no chunk in this launch: nor has any of its threads
                int64_t taken = 0;
                for (int64_t l = blk::walk_next(w); l >= 0; l = blk::walk_next(w)) {
                    if (g < 0 || g >= G) return bad("group", g);
                    if (l < l_begin || l >= l_end) return bad("ladder outside the launch", l);
                    if (blk::block_of(part, l) != k % B) return bad("ladder of another block", l);
                    if (g == 0) {
                        if (seen[(size_t)l]++) return bad("ladder visited twice", l);
                        in_block[(size_t)(k % B)] += 1;
                    }
                    ++taken;
                }
                if (blk::walk_next(w) != -1) return bad("a finished walk went on", t);
                if (taken > cap) return bad("lane over the cap", taken);
                if (t / G >= THREADS / G && taken) return bad("a thread beyond the last whole ladder took one", t);
            }
        }
    }
    // (group 0 stands for all: a thread's ladders do not depend on its group -- checked for the others by the count below)
    for (int64_t l = 0; l < n; ++l)
        if (seen[(size_t)l] != 1) return bad("ladder not visited", l);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (blk::ladders_in_block(part, b, n) != in_block[(size_t)b]) return bad("ladders_in_block", b);
        total += in_block[(size_t)b];
    }
    if (total != n) return bad("total", total);
    return 0;
}

// every group walks the ladders group 0 walks: one small configuration with all groups counted
static int check_groups(int G, int B, int64_t C, int grid, int64_t n, int64_t first)
{
    blk::Part part = {};
    part.l_first = first;
    part.chunk = C;
    part.n_blocks = B;
    std::vector<int> seen((size_t)(n * G), 0);
    for (int k = 0; k < grid; ++k)
        for (int t = 0; t < THREADS; ++t) {
            blk::Walk w;
            const int g = blk::walk_begin(w, part, G, grid, THREADS, k, t, 0, n);
            for (int64_t l = blk::walk_next(w); l >= 0; l = blk::walk_next(w)) seen[(size_t)(l * G + g)] += 1;
        }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) {
            std::printf("FAILED chain %zu visited %d times: G=%d B=%d C=%lld grid=%d ladders=%lld\n", i, seen[i], G, B, (long long)C, grid, (long long)n);
            return 1;
        }
    return 0;
}

int main()
{
    const int Gs[] = {1, 2, 3, 7, 64}, Bs[] = {2, 3, 8, 64}, grids[] = {1, 2, 7};
    const int64_t Cs[] = {1, 5, 36, 37};
    long n_checked = 0;
    for (int G : Gs)
        for (int B : Bs)
            for (int64_t C : Cs) {
                const int64_t counts[] = {1, C - 1, C * B + 1, 30001};
                // shard offsets: none; one that cuts a chunk (unless C = 1); one that puts l_global across 2^32
                const int64_t firsts[] = {0, 3 * C * B + C / 2 + 1, (int64_t(1) << 32) - 7};
                for (int gm : grids)
                    for (int64_t n : counts) {
                        if (n < 1) continue;
                        for (int64_t first : firsts) {
                            // the caps 1, 2, 3 force the launch split; the long count takes them at the widest grid only
                            const int64_t caps[] = {1, 2, 3, 4094};
                            for (int64_t cap : caps) {
                                if (n == 30001 && cap < 3) continue;
                                if (n == 30001 && cap == 3 && gm != 7) continue;
                                if (check(G, B, C, gm * B, n, first, cap)) return 1;
                                ++n_checked;
                            }
                        }
                        if (check_groups(G, B, C, gm * B, n < 2000 ? n : 2000, firsts[1])) return 1;
                    }
            }
    std::printf("ok %ld\n", n_checked);
    return 0;
}
