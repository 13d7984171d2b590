// What the conv kernels' tails share (nn_gemm.hip, nn_conv_halo.hip, nn_conv_ht.hip, nn_conv_sk.hip, nn_conv_rr.hip): the in-launch split-K hand-off
// with the layout of its workspace, the slot address of the epilogues' GroupNorm octet partials, and the bank swizzles of the halo tiles.
// Everything is inlined into its caller: no kernel, no launch and no entry point lives here.  The accumulator staging, the row loops, the slice
// stores / loads of the combine and every main loop stay with their kernel -- those are scheduled per kernel and are not the same code.  So does
// each epilogue's fixed-order column sum of the partials: the same algorithm five times, but behind one inlined definition hipcc scheduled every
// kernel's tail differently (register and instruction counts moved), and a shared form has to be timed kernel by kernel before it may replace them.
#pragma once
#include "nn_common.h"
#include <type_traits>

namespace pdnn {

// ---- host: the split-K workspace.  The first PD_SK_TICKET_FLOATS words are the ticket counters of the in-launch combine (one per output tile, zero at
// allocation, reset by the last arriver of every launch); the payload -- the f32 slices of k_conv_sk / k_conv_rr / k_conv_ht, or the [splits][M][Cout]
// partials of the halo and implicit-GEMM kernels in front of k_splitk_reduce, which must not land on the tickets -- starts behind them.
inline size_t split_payload_floats(size_t ws_floats) { return ws_floats > PD_SK_TICKET_FLOATS ? ws_floats - PD_SK_TICKET_FLOATS : 0; }
struct SplitWs { unsigned* tickets; float* payload; size_t payload_floats; };
inline SplitWs split_ws(float* ws, size_t ws_floats) {
    const size_t pf = ws != nullptr ? split_payload_floats(ws_floats) : 0;
    return SplitWs{reinterpret_cast<unsigned*>(ws), pf ? ws + PD_SK_TICKET_FLOATS : nullptr, pf};
}
// do S slices of `floats_per_tile_and_split` floats for each of `tiles` tiles fit: one ticket word per tile, the slices behind the ticket table
inline bool split_tiles_fit(long long tiles) { return tiles <= PD_SK_TICKET_FLOATS; }
inline bool split_fits(size_t ws_floats, long long tiles, size_t floats_per_tile_and_split, int S) {
    return split_tiles_fit(tiles) && (size_t)tiles * S * floats_per_tile_and_split + PD_SK_TICKET_FLOATS <= ws_floats;
}

// ---- device: small things the halo-tile kernels share
template <int B, int E, typename Fn>
__device__ __forceinline__ void static_for(Fn&& fn) {
    if constexpr (B < E) { fn(std::integral_constant<int, B>{}); static_for<B + 1, E>(fn); }
}
// 16-byte slot swizzles of 64-byte LDS rows (32 channels), mirrored on the LDS-DMA source address: conflict-free ds_read_b128
__device__ __forceinline__ int swz_b(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }   // weight slice: aligned 16-row windows
__device__ __forceinline__ int swz_a(int hp) { return ((hp >> 2) & 1) << 1; }                     // halo: a 16-pixel window starting at any pixel

// ---- device: the in-launch split-K hand-off, the engine's only cross-workgroup protocol.  The S workgroups of a tile have each stored their f32 slice;
// this decides which of them goes on to sum the slices.  Call it from every thread of the workgroup, behind the slice stores; `flag` is a word of the
// caller's LDS that nothing else uses (ONE __shared__ object: cdna guide section 5 trap 4a).  Returns whether this workgroup drew the last ticket.
// Hand-off form R1 of the cdna guide (section 6, guideline 16; microarch "valid forms"): the payload is stored WRITE-THROUGH (sc1: it is in memory, not
// in this XCD's L2, once the store has completed), every storing wave drains with an asm vmcnt(0) the compiler cannot drop, the workgroup joins, and
// only then one lane takes the ticket with a relaxed agent-scope atomic; the last arriver reads the slices with sc1 loads (L1 bypass).  No release /
// acquire fence: a buffer_wbl2 / buffer_inv pair per workgroup measured 3.9x slower in the guide's own table and orders nothing the write-through +
// drain does not.  The last arriver sums ALL slices in slice order, its own included, so the result never depends on who is last.  Contract (pdhip.h,
// pdhip_unet_forward): ONE forward in flight per handle -- tickets and slices live in the handle's workspace.
template <typename Tickets>      // (a reference: the table's address is read by the one lane that uses it, behind the drain)
__device__ __forceinline__ bool splitk_last_arriver(const Tickets& tickets, int tile, int S, int tid, void* flag_word) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains ...
    __syncthreads();                                   // ... before ONE lane takes the ticket
    volatile int* flag = reinterpret_cast<volatile int*>(flag_word);
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == (unsigned)(S - 1);
        if (last) __hip_atomic_store(tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// ---- device: GroupNorm octet partials, layout [img][chunk][Cout / 8][2] = (sum, sum of squares) of the chunk's pixels in channels 8 o .. 8 o + 7.
// Any GroupNorm(32) whose group size is a multiple of 8 channels -- also over a channel concat of two such tensors -- is assembled from these by
// gn_finalize_oct / k_gn_apply without re-reading the tensor.
// n0: first channel of the tile (a multiple of 8), c: octet inside the tile.  (k_conv_sk keeps the expression in its own text: its code changed with the call.)
__device__ __forceinline__ float* gn_part_slot(float* gn_part, long long img, int chunks, int chunk, int Cout, int n0, int c) {
    return gn_part + (((size_t)img * chunks + chunk) * (Cout >> 3) + (n0 >> 3) + c) * 2;
}

}  // namespace pdnn
