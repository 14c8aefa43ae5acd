// Whole doc vectors out of the inverted index (msr_doc_vectors; included by msr_device.hip only). The index is tile-major
// inverted and keeps no forward view of a doc: these kernels rebuild the rows of listed docs by streaming every posting
// of the tiles that hold one, the reverse of the accumulation. Almost every posting belongs to a doc nobody listed, so
// the work per posting is one LDS lookup; only a hit pays for more. The host (docvec_plan, msr_listed_plan.hpp) sorts the
// distinct listed ordinals: row r of the device output is the r-th of them, and the rows of one tile are neighbours.
//
// docvec_tiles<TILE, FILL>  one workgroup of 256 threads per (tile, stripe of kDocvecStripeVecs vecs of the tile's
//                 contiguous vec range [seg_ptr[tile][0], seg_ptr[tile][n_terms])). LDS holds a 16-bit membership map of
//                 the tile, slot[local ordinal] = 1 + index of the doc among the tile's listed docs (0 = not listed; a
//                 byte does not do: all of a tile's up to 32 768 docs may be listed, and 32 768 fits 16 bits). The
//                 lanes stream the stripe with 16-byte loads, four in flight per lane. A posting with weight 0 is
//                 padding and is dropped BEFORE the lookup (its ordinal looks real). Every posting is visited, so the
//                 chunk interleave of a segment need not be undone.
//                   FILL = false (count pass): a hit adds 1 to len[row] (vector atomic on a global counter).
//                   FILL = true  (fill pass):  a hit takes the next free place of its row, pos = atomicAdd(len[row], 1)
//                                (len zeroed again by the host), and stores (term, weight) at ptr[row] + pos. The term
//                                of vec v is the t with seg_row[t] <= v < seg_row[t + 1]: an upper bound over the
//                                tile's seg_ptr row, minus one, which steps over runs of empty segments that share one
//                                start (terms the tile lacks, dense-head terms). The search is narrowed to the terms
//                                of the stripe's first and last vec, found once per workgroup, and runs once per vec
//                                that holds a hit (a vec never straddles two segments).
// docvec_dense<FILL>        one thread per row: both halves of dense[tile][pair][local] for every pair; a slot whose
//                 dense_terms entry is 0xFFFFFFFF (padding of an odd-sized head) is skipped. Same counters.
// docvec_order              one workgroup per row puts the row into ascending term id, out of place (fill order ->
//                 final arrays). A doc holds a term once, so the order is unique and the result does not depend on the
//                 order the atomics of the fill pass arrived in. Rows of up to kDocvecSortRow entries are sorted in LDS
//                 (bitonic network over 64-bit keys term << 32 | weight); a longer row (it may hold all n_terms terms)
//                 takes the slower exact path: entry i goes to place #{j : term_j < term_i}, O(len^2) reads of the row.
#pragma once

#include "msr_listed_plan.hpp"

namespace msr {

struct DocvecArgs {
    const uint32_t* seg_ptr;      // [n_tiles][n_terms + 1] absolute vec index
    const uint32_t* postings;     // vec v of the index lives at postings + (v - vec_base) * 4
    const uint32_t* dense;        // [n_tiles][n_pairs][tile_docs]
    const uint32_t* dense_terms;  // [2 * n_pairs] term id of each dense slot, 0xFFFFFFFF = padding slot
    uint32_t n_pairs;
    uint32_t n_terms;
    uint32_t vec_base;
    uint32_t tile_docs;
    const uint4* work;            // docvec_tiles: {tile, first row, rows, stripe} of workgroup blockIdx.x
    uint32_t row0, n_rows;        // docvec_dense / docvec_order: this launch serves rows [row0, n_rows)
    const uint32_t* ords;         // [rows] ordinal of row r (ascending)
    uint32_t* len;                // [rows] count pass: row lengths; fill pass: next free place of each row
    const uint32_t* ptr;          // [rows + 1] first entry of each row (fill and ordering pass)
    uint32_t* term;               // [entries] fill order
    uint32_t* w;
    uint32_t* out_term;           // [entries] ascending term id inside each row
    uint32_t* out_w;
};

// The term of vec v: the t in [lo, hi] with seg_row[t] <= v < seg_row[t + 1], given seg_row[lo] <= v < seg_row[hi + 1].
__device__ __forceinline__ uint32_t docvec_term_of(const uint32_t* seg_row, uint32_t lo, uint32_t hi, uint32_t v) {
    uint32_t x = lo + 1, y = hi + 1;  // first index in [x, y] whose start is above v (y's is)
    while (x < y) {
        const uint32_t m = (x + y) >> 1;
        if (seg_row[m] <= v)
            x = m + 1;
        else
            y = m;
    }
    return x - 1;
}

// (term, weight) into the next free place of `row`; a place past the row's end (the count pass disagreed) is not written
__device__ __forceinline__ void docvec_put(const DocvecArgs& a, uint32_t row, uint32_t t, uint32_t w) {
    const uint32_t at = a.ptr[row] + atomicAdd(&a.len[row], 1u);
    if (at < a.ptr[row + 1]) {
        a.term[at] = t;
        a.w[at] = w;
    }
}

template <int TILE_DOCS, bool FILL>
__global__ __launch_bounds__(256) void docvec_tiles(const DocvecArgs a) {
    static_assert(TILE_DOCS % 8 == 0 && TILE_DOCS <= 65535, "16-bit map: slot values 1 .. TILE_DOCS");
    constexpr uint32_t NT = 256, UL = 4;  // UL 16-byte loads in flight per lane
    __shared__ __attribute__((aligned(16))) uint16_t slot[TILE_DOCS];
    const uint32_t tid = threadIdx.x;
    const uint4 p = a.work[blockIdx.x];  // one scalar load
    const uint32_t tile = p.x, row0 = p.y, n_r = min(p.z, (uint32_t)TILE_DOCS);

    uint4* const m4 = reinterpret_cast<uint4*>(slot);
    for (uint32_t i = tid; i < (uint32_t)TILE_DOCS / 8u; i += NT) m4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();  // the map is zero before a listed doc marks its slot (another thread zeroed it)
    for (uint32_t i = tid; i < n_r; i += NT) {
        const uint32_t l = min(a.ords[row0 + i] - tile * (uint32_t)TILE_DOCS, (uint32_t)TILE_DOCS - 1u);
        slot[l] = (uint16_t)(i + 1);
    }
    __syncthreads();

    const uint32_t* const seg_row = a.seg_ptr + (uint64_t)tile * (a.n_terms + 1);
    const uint32_t s_end = seg_row[a.n_terms];
    const uint64_t lo64 = (uint64_t)seg_row[0] + (uint64_t)p.w * kDocvecStripeVecs;
    if (lo64 >= s_end) return;
    const uint32_t v_lo = (uint32_t)lo64, n = min(s_end - (uint32_t)lo64, kDocvecStripeVecs);
    uint32_t t_lo = 0, t_hi = 0;  // terms of the stripe's first and last vec
    if (FILL) {
        t_lo = docvec_term_of(seg_row, 0, a.n_terms - 1, v_lo);
        t_hi = docvec_term_of(seg_row, t_lo, a.n_terms - 1, v_lo + n - 1);
    }
    const uint4* const vecs = reinterpret_cast<const uint4*>(a.postings) + ((uint64_t)v_lo - a.vec_base);
    for (uint32_t off = 0; off < n; off += NT * UL) {
        uint4 x[UL];
#pragma unroll
        for (uint32_t u = 0; u < UL; ++u) {
            const uint32_t v = off + u * NT + tid;
            x[u] = v < n ? vecs[v] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (uint32_t u = 0; u < UL; ++u) {
            const uint32_t pp[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
            uint32_t t = 0xFFFFFFFFu;  // term of this vec, looked up at its first hit
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t w = pp[e] >> 16;  // unsigned: weights of 32 768 and above keep their value
                if (w != 0) {                    // padding (weight 0) never reaches the map
                    const uint32_t l = pp[e] & 0xFFFFu;
                    const uint32_t s = l < (uint32_t)TILE_DOCS ? slot[l] : 0u;
                    if (s != 0) {
                        const uint32_t row = row0 + s - 1;
                        if (FILL) {
                            if (t == 0xFFFFFFFFu) t = docvec_term_of(seg_row, t_lo, t_hi, v_lo + off + u * NT + tid);
                            docvec_put(a, row, t, w);
                        } else {
                            atomicAdd(&a.len[row], 1u);
                        }
                    }
                }
            }
        }
    }
}

template <bool FILL>
__global__ __launch_bounds__(256) void docvec_dense(const DocvecArgs a) {
    const uint64_t r64 = (uint64_t)a.row0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r64 >= a.n_rows) return;
    const uint32_t r = (uint32_t)r64, ord = a.ords[r], tile = ord / a.tile_docs, local = ord - tile * a.tile_docs;
    const uint32_t* const col = a.dense + (uint64_t)tile * a.n_pairs * a.tile_docs + local;
    uint32_t c = 0;
    for (uint32_t pr = 0; pr < a.n_pairs; ++pr) {
        const uint32_t v = col[(uint64_t)pr * a.tile_docs];
        const uint32_t ww[2] = {v & 0xFFFFu, v >> 16};
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t t = a.dense_terms[2 * pr + h];
            if (ww[h] == 0 || t == 0xFFFFFFFFu) continue;
            if (FILL)
                docvec_put(a, r, t, ww[h]);
            else
                ++c;
        }
    }
    if (!FILL && c != 0) atomicAdd(&a.len[r], c);
}

__global__ __launch_bounds__(256) void docvec_order(const DocvecArgs a) {
    constexpr uint32_t NT = 256;
    __shared__ uint64_t key[kDocvecSortRow];
    const uint32_t tid = threadIdx.x, r = a.row0 + blockIdx.x;  // (the host keeps row0 + grid within n_rows)
    const uint32_t b0 = a.ptr[r], len = a.ptr[r + 1] - b0;      // workgroup-uniform
    if (len == 0) return;
    if (len > kDocvecSortRow) {  // long row: the place of an entry is the number of smaller terms
        for (uint32_t i = tid; i < len; i += NT) {
            const uint32_t t = a.term[b0 + i];
            uint32_t below = 0;
            for (uint32_t j = 0; j < len; ++j) below += a.term[b0 + j] < t ? 1u : 0u;
            a.out_term[b0 + below] = t;
            a.out_w[b0 + below] = a.w[b0 + i];
        }
        return;
    }
    uint32_t n = 64;
    while (n < len) n <<= 1;  // <= kDocvecSortRow (a power of two)
    for (uint32_t i = tid; i < n; i += NT)
        key[i] = i < len ? ((uint64_t)a.term[b0 + i] << 32) | a.w[b0 + i] : ~0ull;  // padding sorts last
    __syncthreads();
    for (uint32_t k = 2; k <= n; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n; i += NT) {
                const uint32_t o = i ^ j;
                if (o > i) {
                    const uint64_t x = key[i], y = key[o];
                    if ((x > y) == ((i & k) == 0)) {
                        key[i] = y;
                        key[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < len; i += NT) {
        a.out_term[b0 + i] = (uint32_t)(key[i] >> 32);
        a.out_w[b0 + i] = (uint32_t)key[i];
    }
}
static_assert((kDocvecSortRow & (kDocvecSortRow - 1)) == 0 && kDocvecSortRow >= 64, "bitonic network over a power of two");

}  // namespace msr
