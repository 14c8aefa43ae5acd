// Exact ranks of listed docs (msr_rank_docs; included by msr_device.hip only). The search kernels answer "which are
// the best k docs"; these answer "where does THIS doc stand for this query", for any rank up to n_docs. Both phases
// run the search path's accumulation unchanged (msr_accumulate.hpp) and then read the exact u32 scores of one query
// against one doc tile out of LDS:
//
// rank_gather_tiles   one workgroup per (query, tile) pair that holds a listed doc (a target) or the query's `self`
//                     doc; 1-D grid over the host-built pair list, tile-major so that neighbours share the tile.
//                     Writes s(t) = acc[t - doc0] of every listed doc of the pair. Tiles without a listed doc are not
//                     accumulated here.
// rank_count_tiles    one workgroup per (tile, query), grid = (query, tile) like score_tiles. Every wave keeps the
//                     query's targets in registers (lane j = target j: at most MSR_RANK_MAX_TARGETS = 64, one lane
//                     each; redundant per wave like the segment table of accumulate_tile_light — no LDS, no barrier),
//                     reads its accumulators ONCE (rounds x NT ds_read_b128, thread `tid` owning vec r*NT + tid as in
//                     tile_select) and counts, per target with s > 0, the docs of the tile whose key
//                     (score << 32 | ~ordinal) beats the target's: x > s, or x == s on a lower ordinal. One DPP scan
//                     per wave and target, one LDS row per wave, then plain stores of the [tile][entry] partial counts:
//                     no zeroed buffer, no global atomics. No bisection, no candidates, no merge.
// rank_reduce         one thread per listed doc: sums the per-tile counts, takes `self` out and writes the rank.
#pragma once

#include "msr_accumulate.hpp"
#include "msr_listed_plan.hpp"

namespace msr {

struct RankArgs {
    ScoreArgs s;             // what the accumulation reads (part / theta / dump are unused here)
    const uint4* pairs;      // gather: {query, shard-local tile, first item, items (<= 65)}
    const uint2* items;      // gather: {slot in `score`, doc - doc0}
    uint32_t* score;         // [n_entries] s(t) of every listed doc, then [nq] s(self[q])
    const uint32_t* t_ptr;   // [nq + 1] entries of query q = [t_ptr[q], t_ptr[q + 1])
    const uint32_t* t_ord;   // [n_entries] ordinals of the listed docs
    const uint32_t* e_query; // [n_entries] query of each entry
    const uint32_t* self;    // [nq] ordinal that does not count for query q, or kRankNoSelf
    uint32_t* partial;       // [tiles][pe] per-tile counts of this pass
    uint32_t* out_rank;      // [n_entries]
    uint32_t n_entries;
    uint32_t e0;             // this pass ranks entries [e0, e0 + pe)
    uint32_t pe;
    uint32_t n_tiles;
};

// Accumulators + the staging area of accumulate_tile (which the per-wave count rows reuse once it is dead) + the
// SelectScratch the accumulation initialises. No candidate buffer, no thread maxima.
template <int TILE_DOCS, int NT>
struct RankLds {
    static constexpr int kAcc = TILE_DOCS * 4;
    static constexpr int kStage = TileLds<TILE_DOCS, NT, 512>::kStage;
    static constexpr int kRows = (NT / 64) * 64 * 4;  // one row of 64 counts per wave
    static constexpr int kUnion = kStage > kRows ? kStage : kRows;
    static constexpr int kTotal = kAcc + kUnion + (int)sizeof(SelectScratch);
    static_assert(TileLds<TILE_DOCS, NT, 512>::kAcc == kAcc, "the accumulation carves its staging right behind the accumulators");
};

template <int TILE_DOCS, int NT, int U, int MIN_WAVES, bool LIGHT>
__global__ __launch_bounds__(NT, MIN_WAVES) void rank_gather_tiles(const RankArgs a) {
    using L = RankLds<TILE_DOCS, NT>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    const uint32_t* const acc = reinterpret_cast<const uint32_t*>(lds);
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(lds + L::kAcc + L::kUnion);
    const uint32_t tid = threadIdx.x;
    const uint4 p = a.pairs[blockIdx.x];  // one scalar load
    const uint32_t q = p.x, tile_l = p.y;
    const uint64_t doc0 = (uint64_t)(a.s.tile0 + tile_l) * TILE_DOCS;
    const uint32_t ndocs_tile = (uint32_t)min((uint64_t)TILE_DOCS, a.s.n_docs - doc0);
    const int rounds = (int)((ndocs_tile + 4 * NT - 1) / (4 * NT));
    if constexpr (LIGHT)
        accumulate_tile_light<TILE_DOCS, NT>(a.s, q, tile_l, rounds, lds, ss, tid);
    else
        accumulate_tile<TILE_DOCS, NT, U>(a.s, q, tile_l, rounds, lds, ss, tid);
    if (tid < p.w) {  // (the host lists only docs below n_docs: their accumulators lie inside `rounds`)
        const uint2 it = a.items[p.z + tid];
        a.score[it.x] = acc[it.y];
    }
}

template <int TILE_DOCS, int NT, int U, int MIN_WAVES, bool LIGHT>
__global__ __launch_bounds__(NT, MIN_WAVES) void rank_count_tiles(const RankArgs a) {
    using L = RankLds<TILE_DOCS, NT>;
    constexpr int NW = NT / 64;
    constexpr int R = TILE_DOCS / (4 * NT);  // rounds of a full tile: the accumulators of a thread fit its registers
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    const uint4* const a4 = reinterpret_cast<const uint4*>(lds);
    uint32_t* const rows = reinterpret_cast<uint32_t*>(lds + L::kAcc);  // [NW][64], over the dead staging area
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(lds + L::kAcc + L::kUnion);
    uint32_t tid = threadIdx.x;
    const uint32_t tile_l = a.s.tl0 + blockIdx.y;
    const uint32_t q = a.s.q0 + blockIdx.x;
    const uint64_t doc0 = (uint64_t)(a.s.tile0 + tile_l) * TILE_DOCS;
    const uint32_t ndocs_tile = (uint32_t)min((uint64_t)TILE_DOCS, a.s.n_docs - doc0);
    const int rounds = (int)((ndocs_tile + 4 * NT - 1) / (4 * NT));
    const uint32_t eb = a.t_ptr[q], n_t = a.t_ptr[q + 1] - eb;  // scalar loads
    if (n_t == 0) return;  // (workgroup-uniform) a query without listed docs has nothing to count
    // The query's targets, lane j = target j. The general accumulation has registers to spare, so the two loads are in
    // flight across it; the light accumulation of the 8192-doc tile sits at the 64-VGPR edge of its 8 waves per SIMD
    // (two registers held across it spill), so there they are requested afterwards and overlap the read-back only.
    uint32_t t_s = 0, t_o = 0;
    if constexpr (!LIGHT) {
        if ((tid & 63) < n_t) {
            t_s = a.score[eb + (tid & 63)];
            t_o = a.t_ord[eb + (tid & 63)];
        }
    }
    if constexpr (LIGHT)
        accumulate_tile_light<TILE_DOCS, NT>(a.s, q, tile_l, rounds, lds, ss, tid);
    else
        accumulate_tile<TILE_DOCS, NT, U>(a.s, q, tile_l, rounds, lds, ss, tid);
    asm volatile("" : "+v"(tid));  // (nothing of the count phase is computed ahead of the accumulation)
    const uint32_t lane = tid & 63;
    const uint32_t wave = rfl(tid >> 6);
    if constexpr (LIGHT) {
        if (lane < n_t) {
            t_s = a.score[eb + lane];
            t_o = a.t_ord[eb + lane];
        }
    }

    // ---- the accumulators, read once. Rounds past `rounds` were never written and slots past the tile's last real
    // doc are padding: both enter as score 0, which beats no target (a target with s == 0 is skipped).
    uint32_t x[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < rounds) v = a4[r * NT + tid];
        const uint32_t i0 = ((uint32_t)r * NT + tid) * 4u;
        x[r][0] = i0 + 0 < ndocs_tile ? v.x : 0u;
        x[r][1] = i0 + 1 < ndocs_tile ? v.y : 0u;
        x[r][2] = i0 + 2 < ndocs_tile ? v.z : 0u;
        x[r][3] = i0 + 3 < ndocs_tile ? v.w : 0u;
    }
    uint32_t mine = 0;  // lane j: docs of this wave's accumulators that beat target j
    for (uint32_t j = 0; j < n_t; ++j) {
        const uint32_t s = rdl(t_s, j);
        if (s == 0) continue;  // not a hit: rank 0 whatever the counts
        const uint32_t o = rdl(t_o, j);
        // docs with a lower ordinal than the target win a tie: local index below lim  <=>  x >= s counts, else x > s
        const uint32_t lim = (uint64_t)o <= doc0 ? 0u : (uint32_t)min((uint64_t)o - doc0, (uint64_t)TILE_DOCS);
        uint32_t c = 0;
        if (lim == 0 || lim == (uint32_t)TILE_DOCS) {  // (wave-uniform) the target lies in another tile: one threshold
            const uint32_t th = s - (lim ? 1u : 0u);   // unsigned; s >= 1
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) c += x[r][e] > th;
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t i = ((uint32_t)r * NT + tid) * 4u + (uint32_t)e;
                    c += x[r][e] > s - (i < lim ? 1u : 0u);
                }
        }
        const uint32_t tot = rdl(wave_inclusive_scan_u32(c), 63);
        if (lane == j) mine = tot;
    }
    rows[wave * 64 + lane] = mine;
    __syncthreads();
    if (tid < n_t) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += rows[w * 64 + tid];
        a.partial[(uint64_t)tile_l * a.pe + (eb - a.e0) + tid] = sum;
    }
}

// rank(q, t) = 0 when s(t) == 0 or t == self, else 1 + #{d != self : key(d) > key(t)}
__global__ __launch_bounds__(256) void rank_reduce(const RankArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.pe) return;
    const uint32_t e = a.e0 + i;
    const uint32_t s = a.score[e], o = a.t_ord[e];
    const uint32_t q = a.e_query[e];
    const uint32_t sf = a.self[q];
    uint32_t rank = 0;
    if (s != 0 && o != sf) {
        uint32_t beat = 0;
        for (uint32_t t = 0; t < a.n_tiles; ++t) beat += a.partial[(uint64_t)t * a.pe + i];
        if (sf != kRankNoSelf) {
            const uint32_t s_self = a.score[a.n_entries + q];
            beat -= (s_self > s || (s_self == s && sf < o)) ? 1u : 0u;  // self was counted by its tile
        }
        rank = beat + 1;
    }
    a.out_rank[e] = rank;
}

}  // namespace msr
