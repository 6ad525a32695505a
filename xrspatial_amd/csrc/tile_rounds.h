// The schedule of the tile relaxers, without an operator: the geometry of a tile and of the head words,
// the launch that turns a round's flags into the next round's four tile lists, the head / flags / list part of the workspace
// and the host loop over the rounds.  hydrology_fill.hip (fill, flats) and cost_distance.hip (min-plus) each bring their own
// relax kernel; the loop is given a callable that launches one colour of it.
//
// What a relax kernel owes the loop: a block takes its tile from `list[blockIdx.x]` (round 0: list == nullptr, every tile of
// the colour, `across` tiles per row of the colour), adds the cells that fell to head[slot * SLOT_STRIDE] (any of SLOTS
// slots), sets flags[] of the eight tiles around a tile in which a cell fell, and of the tile itself when it stopped at CAP.
// Everything sits in an unnamed namespace: a unit that includes this gets its own copy of the kernel in its code object.
#pragma once
#include "xrs_common.h"
#include "workspace.h"

#include <chrono>

namespace xrs {
namespace {

constexpr int TILE = XRS_FILL_TILE;             // 64
constexpr int THREADS = 256;                    // four waves
constexpr int STRIP = TILE / 4;                 // rows of a thread's strip
constexpr int LD = TILE + 2;                    // lanes read adjacent words of a row: no bank conflict at any pitch
constexpr int HALO = 4 * TILE + 4;
constexpr int CAP = 128;                        // in-tile iterations per launch
constexpr int SLOTS = 64, SLOT_STRIDE = 64;
constexpr int TOTAL_WORD = SLOTS * SLOT_STRIDE; // the round's fallen cells, then the four list lengths of the next round
constexpr int COUNT_WORD = TOTAL_WORD + 1;
constexpr int HEAD_WORDS = TOTAL_WORD + 64;
constexpr int ROUNDS_KEPT = XRS_FILL_STATUS_ROUNDS;
static_assert(TILE == 64 && STRIP == 16, "a wave's lanes are a tile's columns");
static_assert(8 + 3 * ROUNDS_KEPT <= XRS_FILL_STATUS_WORDS, "status layout");

struct Offsets {
    unsigned at[4];
};

// the flags of this round -> the four tile lists of the next one; the round's total
__global__ void __launch_bounds__(THREADS) next_lists_kernel(unsigned tiles, unsigned tiles_x, unsigned *__restrict__ flags,
                                                             unsigned *__restrict__ list, Offsets off, unsigned *__restrict__ head) {
    const unsigned tile = blockIdx.x * THREADS + threadIdx.x;
    if (tile < tiles && flags[tile] != 0u) {
        flags[tile] = 0u;
        const unsigned ti = tile / tiles_x, tj = tile - ti * tiles_x;
        const unsigned c = ((ti & 1u) << 1) | (tj & 1u);
        list[off.at[c] + atomicAdd(head + COUNT_WORD + c, 1u)] = tile;
    }
    if (blockIdx.x == 0 && threadIdx.x < SLOTS) {
        const unsigned v = head[threadIdx.x * SLOT_STRIDE];
        if (v != 0u) atomicAdd(head + TOTAL_WORD, v);
    }
}

inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the part of a relaxer's workspace that the rounds use; a caller's carve() takes it first and its own parts behind it
struct RoundWork {
    unsigned *head, *flags, *list;
};
inline RoundWork carve_rounds(Carver &c, size_t rows, size_t cols) {
    const size_t tiles = ((rows + TILE - 1) / TILE) * ((cols + TILE - 1) / TILE);
    RoundWork w = {};
    w.head = c.take<unsigned>(HEAD_WORDS);
    w.flags = c.take<unsigned>(tiles);
    w.list = c.take<unsigned>(tiles);
    return w;
}

// the rounds: status words 0 (rounds run), 1 (tiles launched), 8 + k, 8 + KEPT + k, 8 + 2 KEPT + k (fallen cells, tiles, ns).
// launch_colour(colour, blocks, across, tiles_y, tiles_x, list) enqueues the relax kernel for one colour on `s`.
template <typename LaunchColour>
int run_tile_rounds(const char *what, long rows, long cols, const RoundWork &wk, int64_t *status, bool timed, hipStream_t s,
                    LaunchColour &&launch_colour) {
    const unsigned tiles_y = (unsigned)((rows + TILE - 1) / TILE), tiles_x = (unsigned)((cols + TILE - 1) / TILE);
    const unsigned tiles = tiles_y * tiles_x;                            // at most 2^26: a row or a column of tiles of one cell each
    const unsigned ny[2] = {(tiles_y + 1) / 2, tiles_y / 2}, nx[2] = {(tiles_x + 1) / 2, tiles_x / 2};
    unsigned count[4];
    Offsets off;
    for (unsigned c = 0, at = 0; c < 4; ++c) {
        count[c] = ny[c >> 1] * nx[c & 1];
        off.at[c] = at;
        at += count[c];
    }
    const uint64_t bound = (uint64_t)rows * (uint64_t)cols + 1;          // a round that moves anything brings one more cell to its last value
    XRS_HIP(hipMemsetAsync(wk.flags, 0, (size_t)tiles * 4, s));
    int64_t launched_all = 0;
    for (uint64_t round = 0;; ++round) {
        int64_t t0 = 0;
        if (timed) { XRS_HIP(hipStreamSynchronize(s)); t0 = now_ns(); }
        XRS_HIP(hipMemsetAsync(wk.head, 0, (size_t)HEAD_WORDS * 4, s));
        int64_t launched = 0;
        for (int c = 0; c < 4; ++c) {
            if (!count[c]) continue;
            launch_colour(c, count[c], nx[c & 1], tiles_y, tiles_x, round ? wk.list + off.at[c] : (const unsigned *)nullptr);
            XRS_LAUNCH_CHECK();
            launched += count[c];
        }
        hipLaunchKernelGGL(next_lists_kernel, dim3((tiles + THREADS - 1) / THREADS), dim3(THREADS), 0, s, tiles, tiles_x, wk.flags, wk.list, off,
                           wk.head);
        XRS_LAUNCH_CHECK();
        unsigned words[5] = {0, 0, 0, 0, 0};
        XRS_HIP(hipMemcpyAsync(words, wk.head + TOTAL_WORD, sizeof(words), hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        launched_all += launched;
        status[0] = (int64_t)(round + 1);
        status[1] = launched_all;
        if (round < (uint64_t)ROUNDS_KEPT) {
            status[8 + round] = words[0];
            status[8 + ROUNDS_KEPT + round] = launched;
            if (timed) status[8 + 2 * ROUNDS_KEPT + round] = now_ns() - t0;
        }
        if (words[0] == 0) return 0;
        if (round + 1 >= bound) return fail("%s: no fixed point after rows * cols + 1 = %llu rounds", what, (unsigned long long)bound);
        for (int c = 0; c < 4; ++c) count[c] = words[1 + c];
    }
}

}  // namespace
}  // namespace xrs
