// score_tiles_walk: ONE workgroup per query walks the handle's doc tiles one after the other (included by
// msr_device.hip only; routing rule: walk_route, msr_device_internal.hpp). The name starts with score_tiles: the scorer's
// figures in bench.py and profiles/ are those of the kernels matching that name.
//
// Small indexes (2-8 tiles: the reference's Flickr30K and COCO corpora) spend most of score_tiles' life on work that is
// the same for every tile of a query: the kernel arguments, q_meta, the query's terms, weights and dense-head weights,
// the lane constants — repeated per (tile, query) workgroup and per wave — and then hand k keys per tile through HBM to
// two merge launches. Here the query side (LightQuery) is loaded once per workgroup, the tile side of every step is one
// scalar load from the handle's per-tile table (WalkTile), and the running top-k `best` stays in LDS:
//     tile 0      accumulate (light_init + LightChunks, msr_accumulate.hpp), tile_select -> best
//     tile t > 0  accumulate; theta = best[k-1] is a lower bound on the final k-th key, so the tile only has to
//                 report keys at or above it: the candidate buffer is seeded with best's k keys, theta_select appends
//                 the tile's survivors and ranks the lot back into best. While best is not full (theta = 0), or when
//                 more keys survive than the buffer holds (mass ties), the tile runs the full tile_select into `side`
//                 and wave 0 merges the two sorted lists. Exact either way.
//     end         wave 0 writes the result rows by merge_wave's rule (emit_ranked).
// The tiles share ONE accumulator carve (TileLds, as score_tiles) — never all tiles at once — so four workgroups
// (32 waves) per CU stay resident at 8192 docs per tile. Three barriers per tile, as in score_tiles.
#pragma once

#include "msr_kernels.hpp"

namespace msr {

// A structure that no kernel writes, read through the constant address space: the wave-uniform load is then a scalar
// one wherever it stands in the loop.
template <class T>
__device__ __forceinline__ T load_uniform(const T* p) {
    static_assert(sizeof(T) % 4 == 0, "whole dwords");
    const __attribute__((address_space(4))) uint32_t* w = (const __attribute__((address_space(4))) uint32_t*)p;
    T out;
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 4; ++i) reinterpret_cast<uint32_t*>(&out)[i] = w[i];
    return out;
}

// best (k keys, best first, empty slots last) <- the k best of best and side; both lists hold unique keys. One wave.
__device__ __forceinline__ void merge_best(uint64_t* best, const uint64_t* side, const uint32_t k, const uint32_t lane) {
    const uint64_t x = lane < k ? best[lane] : 0ull, y = lane < k ? side[lane] : 0ull;
    uint32_t rx = lane, ry = lane;  // rank inside the own list = slot
    for (uint32_t j = 0; j < k; ++j) {
        rx += side[j] > x;
        ry += best[j] > y;
    }
    // (every lane has read both lists; the non-empty keys take ranks 0 .. n-1, and the slots from n on were empty in best)
    if (x != 0 && rx < k) best[rx] = x;
    if (y != 0 && ry < k) best[ry] = y;
}

template <int TILE_DOCS, int NT, int MIN_WAVES>
__global__ __launch_bounds__(NT, MIN_WAVES) void score_tiles_walk(const WalkArgs a) {
    constexpr int CAND = 512;
    using L = TileLds<TILE_DOCS, NT, CAND>;
    static_assert(TILE_DOCS / (4 * NT) <= (int)kWalkRoundsMask, "rounds share a word with doc0");
    static_assert(L::kTotal + 2 * 64 * 8 <= 40960, "four workgroups of the 8192-doc shape per CU");

    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    __shared__ uint64_t best[kWalkMaxK], side[kWalkMaxK];
    uint8_t* const un = lds + L::kAcc;
    const uint4* const a4 = reinterpret_cast<const uint4*>(lds);
    uint64_t* const cand = reinterpret_cast<uint64_t*>(un);
    uint32_t* const tmax = reinterpret_cast<uint32_t*>(un + L::kUnion);
    uint32_t* const wmax = tmax + NT;
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(un + L::kUnion + L::kTmax);

    const uint32_t q = blockIdx.x;
    const uint32_t k = a.m.k;
    __builtin_assume(k >= 1 && k <= kWalkMaxK);  // (launch_walk refuses any other: the selection's k > 64 branches go)
    uint32_t tid = threadIdx.x;
    LightQuery lq = load_light_query(a.s, q, tid & 63);  // once per workgroup: the same for every tile

    // Software pipeline over the tiles: nothing of a tile's (segment lookup -> scan -> first UL chunk loads per wave)
    // chain depends on the tile before it, so tile t+1's chain runs while tile t is finished and selected, and its
    // postings are in registers when tile t+1's accumulators are initialised. Tile 0 is primed here.
    LightChunks<NT / 64> ch;
    // (of a tile's table row only the dense-head rows and the doc range are carried into its own iteration: what the
    // lookup and the requests need is used where the row is loaded)
    const char* dense;
    uint32_t doc0_rounds;
    {
        const WalkTile wt = load_uniform(a.tiles);  // one scalar load per tile: no address arithmetic per wave and tile
        dense = wt.dense;
        doc0_rounds = wt.doc0_rounds;
        ch.lookup(lq, (global_u32)wt.seg_row, tid & 63);
        ch.scan(wt.tile_first, rfl(tid >> 6));
        ch.request(lq, wt.post_base, 0, rfl(tid >> 6), tid & 63);
    }

    for (uint32_t tl = 0; tl < a.n_tiles; ++tl) {
        // a per-tile copy of the thread id: what the tile's phases derive from it (accumulator addresses, doc keys) is
        // recomputed where it is used instead of being hoisted out of the loop into registers the kernel does not have
        asm volatile("" : "+v"(tid), "+v"(lq.s_t), "+v"(lq.s_w), "+v"(lq.qv));
        LightTile lt;
        lt.dense = dense;
        lt.dense_bytes = a.s.n_pairs * (uint32_t)(TILE_DOCS * 4);
        lt.rounds = min((int)(doc0_rounds & kWalkRoundsMask), TILE_DOCS / (4 * NT));
        const uint64_t doc0 = doc0_rounds & ~kWalkRoundsMask;
        const bool more = tl + 1 < a.n_tiles;  // the last tile requests nothing
        uint32_t* const acc = reinterpret_cast<uint32_t*>(lds);
        const uint32_t lane = tid & 63, wave = rfl(tid >> 6);

        light_init<TILE_DOCS, NT>(lq, lt, reinterpret_cast<uint4*>(lds), tid, [] {});
        // every wave has left the previous tile's selection: its ranking of `best` is complete and visible, and
        // nobody reads the candidate buffer or the scratch of that tile any more
        __syncthreads();
        uint64_t theta = 0;
        if (tl) {
            const uint64_t th = best[k - 1];  // 0: fewer than k hits so far
            theta = ((uint64_t)rfl((uint32_t)(th >> 32)) << 32) | rfl((uint32_t)th);
        }
        if (tid < 64) {
            ss.cnt[tid] = 0;
            if (theta && tid < k) cand[tid] = best[tid];
        }
        if (tid == 0) {
            uint32_t one = 1;  // (made here, behind an opaque copy: not a constant held in a register across the tiles)
            asm volatile("" : "+v"(one));
            ss.n_cand = theta ? k : 0u;
            ss.tau0 = one;
            ss.smax = one - 1;
        }
        ch.add(acc, lane);  // the chunks requested before the previous tile's selection (before the loop: tile 0)
        if (ch.count_w > ch.UL) {  // rare
            const WalkTile wt = load_uniform(a.tiles + tl);
            lt.seg_row = (global_u32)wt.seg_row;
            lt.tile_first = wt.tile_first;
            lt.post_base = wt.post_base;
            ch.add_leftover(lq, lt, acc, wave, lane);
        }
        // the next tile's segment bounds: requested once this wave's LDS adds are out, so that the wait at the barrier
        // covers the round trip
        // (the row is loaded unconditionally — the last tile re-reads its own — so that it stays in scalar registers)
        const WalkTile nx = load_uniform(a.tiles + min(tl + 1, a.n_tiles - 1));
        if (more) ch.lookup(lq, (global_u32)nx.seg_row, lane);
        __syncthreads();  // accumulation complete
        // ... and its first chunks: the selection's passes and the ranking cover the postings' latency
        if (more) {
            ch.scan(nx.tile_first, wave);
            ch.request(lq, nx.post_base, 0, wave, lane);
        }
        dense = nx.dense;
        doc0_rounds = nx.doc0_rounds;

        if (theta && theta_select<TILE_DOCS, NT, CAND>(a4, cand, ss, lt.rounds, doc0, (int)k, best, theta, tid)) continue;
        tile_select<TILE_DOCS, NT, CAND>(a4, cand, tmax, wmax, ss, lt.rounds, doc0, (int)k, tl ? side : best, tid);
        if (tl) {
            __syncthreads();  // `side` is complete
            if (tid < 64) merge_best(best, side, k, tid);
        }
    }
    __syncthreads();  // `best` is final
    // (the result pointers are read from the kernel-argument segment only now — behind an opaque copy of its address —
    // instead of being held in ten scalar registers through the loop)
    uint64_t ka = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const MergeArgs m = load_uniform(reinterpret_cast<const MergeArgs*>(ka + offsetof(WalkArgs, m)));
    if (tid < 64) emit_ranked(m, q, tid, tid < k ? best[tid] : 0ull, tid);
}

}  // namespace msr
