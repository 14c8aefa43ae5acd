// Filtered search (msr_search_filtered, msr_dense_search_filtered; included by msr_filter.hip only): "search, but only
// among these docs". Every query names one of the call's doc sets (FilterArgs, msr_device_internal.hpp), a bitmap over
// doc ordinals (sparse route) or rows (dense route); the hits of the query are the members of its set. Counterpart:
// Lucene's filter queries, which the reference never issues (its COCO 1K folds are separate indexes).
//
// The tile kernels hold a whole tile's exact scores in LDS before they select, and a score / key of 0 means "no hit"
// to every selector and merge downstream. A filter is therefore ONE masking step between accumulation and selection:
//
// score_tiles_filtered<TILE_DOCS, NT, U, MIN_WAVES, CAND, LIGHT>   score_tiles (msr_kernels.hpp) restated with two additions:
//     1. early exit: a (tile, query) whose set holds no doc of the tile (the host's any[set][tile] byte) writes k empty
//        keys to its row of `part` (the merge reads every list) and leaves before the first barrier; the branch is
//        uniform across the workgroup;
//     2. mask: after accumulate_tile / accumulate_tile_light (which end with a barrier and leave SelectScratch
//        initialised) thread `tid` ANDs each of its vecs a4[r * NT + tid] with the four bits of its docs, then a barrier
//        (the histogram and theta paths read vecs that other threads masked); theta_select / tile_select run unchanged.
//     Queries with q_set = -1 skip both. There is no dump instance: the instances are light with the 512-key buffer,
//     k <= 512, and the 1024-key buffer.
// select_tiles_filtered<TILE_DOCS, NT, CAND>   select_tiles whose load from the key matrix into LDS applies the same mask
//     (filter_mask4), with the same early exit. The dense search runs in passes of queries: `part` rows are pass-local
//     ([tile][a.qn][k], row qi), q_set is indexed by the call's query a.q0 + qi.
//
// score_dump_filtered<TILE_DOCS, NT, U, MIN_WAVES, LIGHT>   the dump instance of score_tiles (MODE 1, dump_add = 0, every
//     tile; msr_hybrid_deep_filtered's sparse score rows) with the same two additions, adapted to a dump:
//     1. early exit: the skipped (tile, query) writes ZEROS to exactly the rounds * NT vecs of its dump segment that the
//        unfiltered dump writes (the score rows live in reused scratch: a skipped segment would otherwise keep the scores
//        of an earlier call or pass) and leaves before the first barrier;
//     2. mask: thread `tid` reads its vec a4[r * NT + tid] after the accumulation, masks it in registers and stores it to
//        the dump: no write back to LDS, no extra barrier.
// mask_key_rows   elementwise and in place over the dense key rows D[row][ld] of one msr_hybrid_deep_filtered pass (column =
//     doc ordinal): a non-member's key becomes 0. Grid = (column blocks, rows), 256 threads, 16-byte loads and stores, a
//     wave covering 1 KiB of a row (fuse_rows' access shape); vec i of a row takes bits (i & 7) * 4 .. of word i >> 3 of
//     the set's bitmap row, which holds n_tiles * tile_docs / 32 >= ld / 32 zero-padded words (the host checks it), so
//     every vec up to ld is read in bounds and columns at or above n come out 0. The row's set is q_set[q0 + row], the
//     CALL's query; a workgroup of an unfiltered row returns at once.
//
// Why nothing else of msr_hybrid_deep changes (deep_select_rows, fuse_rows, gather_src run as they are): once both rows
// are masked, a non-member's dense key is 0 and its sparse score is 0. deep_select_rows takes key 0 as "no member", so
// both depth lists are the exact top-depth of the set's docs. In fuse_rows a doc is in the sparse list only with s != 0
// (in_s is false for a masked doc), and in the dense list only with a key at or above the list's last key, which is
// non-zero in any non-empty dense list because f32_to_key gives no finite score the key 0 (in_d is false for a masked
// doc; an empty list admits nobody). So no masked doc is a member, has a source bit or is counted, and the extremes are
// those of the two filtered lists: the result is what an index holding only the set's docs would give.
//
// The values a workgroup derives from its query (q_set[q], the any byte, the set's row base) are wave-uniform: they
// come from blockIdx and go through v_readfirstlane, so the bitmap row base stays in SGPRs and the early-exit branch
// is scalar.
#pragma once

#include "msr_accumulate.hpp"

namespace msr {

// Vec v of a tile (docs 4v .. 4v+3 of the tile) masked by the query's set: `row_tile` is the set's bitmap row at the
// tile's first word. A tile starts on a multiple of 4096 docs, so the four bits of a vec never straddle a word.
__device__ __forceinline__ uint4 filter_mask4(const uint32_t* __restrict__ row_tile, const uint32_t v, uint4 x) {
    const uint32_t m = row_tile[v >> 3] >> ((v & 7u) * 4u);
    x.x = (m & 1u) ? x.x : 0u;
    x.y = (m & 2u) ? x.y : 0u;
    x.z = (m & 4u) ? x.z : 0u;
    x.w = (m & 8u) ? x.w : 0u;
    return x;
}

// The set of query q (-1: unfiltered), wave-uniform.
__device__ __forceinline__ int32_t filter_set_of(const FilterArgs& f, const uint32_t q) { return (int32_t)rfl((uint32_t)f.q_set[q]); }
// Does set `set` (>= 0) hold a doc of global tile `tile_g`? Wave-uniform.
__device__ __forceinline__ bool filter_tile_live(const FilterArgs& f, const int32_t set, const uint32_t tile_g) {
    return rfl((uint32_t)f.any[(uint64_t)(uint32_t)set * f.n_tiles + tile_g]) != 0u;
}
// The set's bitmap row at the first word of global tile `tile_g` (tile_docs / 32 words per tile).
__device__ __forceinline__ const uint32_t* filter_row_tile(const FilterArgs& f, const int32_t set, const uint32_t tile_g,
                                                            const uint32_t tile_words) {
    return f.bits + (uint64_t)(uint32_t)set * f.stride + (uint64_t)tile_g * tile_words;
}

// <docs per tile, threads, 1-KiB chunk loads per register bank, min waves per SIMD, candidate-key capacity (>= k),
// light accumulation>: the template parameters of score_tiles without its MODE.
template <int TILE_DOCS, int NT, int U, int MIN_WAVES, int CAND, bool LIGHT = false>
__global__ __launch_bounds__(NT, MIN_WAVES) void score_tiles_filtered(const ScoreArgs a, const FilterArgs f) {
    using L = TileLds<TILE_DOCS, NT, CAND>;

    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    uint32_t* const acc = reinterpret_cast<uint32_t*>(lds);
    uint8_t* const un = lds + L::kAcc;
    uint64_t* const cand = reinterpret_cast<uint64_t*>(un);
    uint32_t* const tmax = reinterpret_cast<uint32_t*>(un + L::kUnion);
    uint32_t* const wmax = tmax + NT;
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(un + L::kUnion + L::kTmax);

    const uint32_t tid = threadIdx.x;
    const uint32_t tile_l = a.tl0 + blockIdx.y;
    const uint32_t q = a.q0 + blockIdx.x;
    const uint32_t tile_g = a.tile0 + tile_l;
    const uint64_t doc0 = (uint64_t)tile_g * TILE_DOCS;
    const uint32_t ndocs_tile = (uint32_t)min((uint64_t)TILE_DOCS, a.n_docs - doc0);
    const int rounds = (int)((ndocs_tile + 4 * NT - 1) / (4 * NT));
    uint4* const a4 = reinterpret_cast<uint4*>(acc);
    uint64_t* out = a.part + ((uint64_t)tile_l * a.nq + q) * a.k;
    const int k = (int)a.k;

    // ---- early exit: the query's set holds no doc of this tile (uniform across the workgroup, before any barrier)
    const int32_t set = filter_set_of(f, q);
    if (set >= 0 && !filter_tile_live(f, set, tile_g)) {
        for (int i = (int)tid; i < k; i += NT) out[i] = empty_key();
        return;
    }

    const uint64_t theta = a.theta ? a.theta[(uint64_t)q * a.k + (a.k - 1)] : 0ull;
    if constexpr (LIGHT)
        accumulate_tile_light<TILE_DOCS, NT>(a, q, tile_l, rounds, lds, ss, tid);
    else
        accumulate_tile<TILE_DOCS, NT, U>(a, q, tile_l, rounds, lds, ss, tid);

    // ---- mask: a non-member's score becomes 0 = "no hit"
    if (set >= 0) {
        const uint32_t* const row_tile = filter_row_tile(f, set, tile_g, TILE_DOCS / 32);
        for (int r = 0; r < rounds; ++r) {
            const uint32_t v = (uint32_t)r * NT + tid;
            a4[v] = filter_mask4(row_tile, v, a4[v]);
        }
        __syncthreads();  // the selection reads vecs that other threads masked
    }

    if (theta && theta_select<TILE_DOCS, NT, CAND>(a4, cand, ss, rounds, doc0, k, out, theta, tid)) return;
    tile_select<TILE_DOCS, NT, CAND>(a4, cand, tmax, wmax, ss, rounds, doc0, k, out, tid, false);
}

// select_tiles over the dense route's key matrix, src[qi * n_tiles * TILE_DOCS + row]; grid = (query of the pass, tile).
// a.tpr = a.n_tiles (one "rank" owns every tile), a.q0 = the pass's first query in the call.
template <int TILE_DOCS, int NT, int CAND>
__global__ __launch_bounds__(NT) void select_tiles_filtered(const SelectArgs a, const FilterArgs f) {
    using L = TileLds<TILE_DOCS, NT, CAND>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    uint4* const a4 = reinterpret_cast<uint4*>(lds);
    uint8_t* const un = lds + L::kAcc;
    uint64_t* const cand = reinterpret_cast<uint64_t*>(un);
    uint32_t* const tmax = reinterpret_cast<uint32_t*>(un + L::kUnion);
    uint32_t* const wmax = tmax + NT;
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(un + L::kUnion + L::kTmax);
    const uint32_t tid = threadIdx.x;
    const uint32_t t = blockIdx.y, qi = blockIdx.x;  // t < a.n_tiles: the launcher's grid
    uint64_t* out = a.part + ((uint64_t)t * a.qn + qi) * a.k;
    const int32_t set = filter_set_of(f, a.q0 + qi);
    if (set >= 0 && !filter_tile_live(f, set, t)) {
        for (uint32_t i = tid; i < a.k; i += NT) out[i] = empty_key();
        return;
    }
    const uint64_t doc0 = (uint64_t)t * TILE_DOCS;
    const uint32_t ndocs_tile = (uint32_t)min((uint64_t)TILE_DOCS, a.n_docs - doc0);
    const int rounds = (int)((ndocs_tile + 4 * NT - 1) / (4 * NT));
    const uint4* src = reinterpret_cast<const uint4*>(a.src + ((uint64_t)qi * a.tpr + t) * TILE_DOCS);
    if (set >= 0) {
        const uint32_t* const row_tile = filter_row_tile(f, set, t, TILE_DOCS / 32);
        for (int r = 0; r < rounds; ++r) {
            const uint32_t v = (uint32_t)r * NT + tid;
            a4[v] = filter_mask4(row_tile, v, src[v]);
        }
    } else {
        for (int r = 0; r < rounds; ++r) a4[r * NT + tid] = src[r * NT + tid];
    }
    if (tid < 64) ss.cnt[tid] = 0;
    if (tid == 0) {
        ss.n_cand = 0;
        ss.tau0 = 1;
        ss.smax = 0;
    }
    __syncthreads();
    tile_select<TILE_DOCS, NT, CAND>(a4, cand, tmax, wmax, ss, rounds, doc0, (int)a.k, out, tid, false);
}

// The dump instance of score_tiles under a filter: grid = (query of the pass, tile), a.dump_add = 0, a.part unused.
// <docs per tile, threads, chunk loads per bank, min waves per SIMD, light accumulation>; LDS is the dump instance's
// (TileLds with the 512-key union: the accumulation's staging arrays live there).
template <int TILE_DOCS, int NT, int U, int MIN_WAVES, bool LIGHT = false>
__global__ __launch_bounds__(NT, MIN_WAVES) void score_dump_filtered(const ScoreArgs a, const FilterArgs f) {
    using L = TileLds<TILE_DOCS, NT, 512>;

    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    uint8_t* const un = lds + L::kAcc;
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(un + L::kUnion + L::kTmax);

    const uint32_t tid = threadIdx.x;
    const uint32_t tile_l = a.tl0 + blockIdx.y;
    const uint32_t q = a.q0 + blockIdx.x;
    const uint32_t tile_g = a.tile0 + tile_l;
    const uint64_t doc0 = (uint64_t)tile_g * TILE_DOCS;
    const uint32_t ndocs_tile = (uint32_t)min((uint64_t)TILE_DOCS, a.n_docs - doc0);
    const int rounds = (int)((ndocs_tile + 4 * NT - 1) / (4 * NT));
    const uint4* const a4 = reinterpret_cast<const uint4*>(lds);
    const uint32_t g = tile_g / a.tpr, t = tile_g % a.tpr;
    uint4* const dst = reinterpret_cast<uint4*>(a.dump + (((uint64_t)g * a.qn + (q - a.q0)) * a.tpr + t) * TILE_DOCS);

    // ---- early exit: the set holds no doc of this tile; the segment is zeroed, not left as it was
    const int32_t set = filter_set_of(f, q);
    if (set >= 0 && !filter_tile_live(f, set, tile_g)) {
        for (int r = 0; r < rounds; ++r) dst[r * NT + tid] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }

    if constexpr (LIGHT)
        accumulate_tile_light<TILE_DOCS, NT>(a, q, tile_l, rounds, lds, ss, tid);
    else
        accumulate_tile<TILE_DOCS, NT, U>(a, q, tile_l, rounds, lds, ss, tid);

    // ---- the dump, masked on its way out: thread `tid` owns vec r * NT + tid (conflict-free ds_read_b128)
    if (set >= 0) {
        const uint32_t* const row_tile = filter_row_tile(f, set, tile_g, TILE_DOCS / 32);
        for (int r = 0; r < rounds; ++r) {
            const uint32_t v = (uint32_t)r * NT + tid;
            dst[v] = filter_mask4(row_tile, v, a4[v]);
        }
    } else {
        for (int r = 0; r < rounds; ++r) dst[r * NT + tid] = a4[r * NT + tid];
    }
}

constexpr int kMaskRowsThreads = 256;
constexpr int kMaskRowsVecs = 2;                                      // vecs of 4 columns per thread
constexpr int kMaskRowsCols = kMaskRowsThreads * kMaskRowsVecs * 4;   // columns per workgroup

struct MaskRowsArgs {
    uint32_t* D;    // [rows][ld] keys, column = doc ordinal; 16-byte aligned
    uint64_t ld;    // a multiple of 4, at most 32 * f.stride
    uint32_t q0;    // the pass's first query in the call: row r belongs to query q0 + r
    FilterArgs f;   // (any / n_tiles unused)
};

__global__ __launch_bounds__(kMaskRowsThreads) void mask_key_rows(const MaskRowsArgs a) {
    const uint32_t row = blockIdx.y;
    const int32_t set = filter_set_of(a.f, a.q0 + row);
    if (set < 0) return;  // (uniform across the workgroup)
    const uint32_t* const bits = a.f.bits + (uint64_t)(uint32_t)set * a.f.stride;
    uint4* const D = reinterpret_cast<uint4*>(a.D + (uint64_t)row * a.ld);
    const uint32_t nv = (uint32_t)(a.ld / 4);
    uint32_t i[kMaskRowsVecs];
    uint4 x[kMaskRowsVecs];
#pragma unroll
    for (int v = 0; v < kMaskRowsVecs; ++v) {  // loads first
        i[v] = (blockIdx.x * kMaskRowsVecs + (uint32_t)v) * kMaskRowsThreads + threadIdx.x;
        if (i[v] < nv) x[v] = D[i[v]];
    }
#pragma unroll
    for (int v = 0; v < kMaskRowsVecs; ++v)
        if (i[v] < nv) D[i[v]] = filter_mask4(bits, i[v], x[v]);
}

}  // namespace msr
