// Per-term doc weights of listed docs (msr_explain_docs; included by msr_device.hip only). The search and rank kernels
// return sums; this one returns the addends: for a listed doc t and a query entry (tau, omega) the stored weight
// w(tau, t), read straight out of the index. It shares no code with the accumulation (msr_accumulate.hpp): segments
// and dense rows are addressed here on their own, so  sum_j omega_j * w(tau_j, t) == msr_rank_docs' score  compares two
// independent walks over the same bytes.
//
// explain_tiles   one workgroup of 256 threads per (query, tile) pair that holds a listed doc; 1-D grid over the
//                 host-built pair list, tile-major so that neighbours share the tile in L2 (as rank_gather_tiles).
//                 LDS holds a byte map of the tile, slot[local ordinal] = 1 + index of the listed doc (0 = not listed;
//                 at most MSR_EXPLAIN_MAX_TARGETS = 64 listed docs per query, duplicates collapsed by the host), and
//                 the row of each listed doc in the output. The four waves take the query's counting entries
//                 round-robin:
//                   sparse term      the lanes stream the vecs of segment [seg_ptr[tile][tau], seg_ptr[tile][tau + 1])
//                                    with 16-byte loads, four in flight per lane; a posting with weight != 0 looks its
//                                    local ordinal up in the byte map and, on a hit, stores its weight. Padding postings
//                                    carry weight 0 and are dropped BEFORE the lookup (their ordinals look real). Every
//                                    posting is visited, so the chunk interleave of a segment need not be undone.
//                   dense-head term  lane j < listed docs reads dense[tile][pair][local ordinal of doc j] and stores the
//                                    term's half when it is not 0.
//                 A (doc, entry) slot is written by at most one lane of one workgroup (a doc holds a term once; every
//                 input entry, a repeated term included, owns its slot), so the stores are plain vector stores: no
//                 atomics. The output is zeroed once by the host (hipMemsetAsync): slots of entries that do not count
//                 and of terms the doc lacks are never written.
#pragma once

#include "msr_listed_plan.hpp"
#include "msr_select.hpp"

namespace msr {

struct ExplainArgs {
    const uint32_t* seg_ptr;   // [n_tiles][n_terms + 1] absolute vec index
    const uint32_t* postings;  // vec v of the index lives at postings + (v - vec_base) * 4
    const uint32_t* dense;     // [n_tiles][n_pairs][TILE_DOCS]
    uint32_t n_pairs;
    uint32_t n_terms;
    uint32_t vec_base;
    const uint4* pairs;        // {query, tile, first item, items (<= 64)}
    const uint2* items;        // {first output slot of the doc's row, doc - doc0}
    const uint2* q_range;      // [nq] counting entries of query q = ents[x .. y)
    const uint2* ents;         // {term id | kExplainDense + dense slot, slot of the entry inside a row}
    uint32_t* out;
};

template <int TILE_DOCS>
__global__ __launch_bounds__(256) void explain_tiles(const ExplainArgs a) {
    static_assert(TILE_DOCS % 16 == 0 && TILE_DOCS <= 65536, "byte map: one byte per 16-bit local ordinal");
    constexpr uint32_t NT = 256, NW = NT / 64, UL = 4;  // UL 16-byte loads in flight per lane
    __shared__ __attribute__((aligned(16))) uint8_t slot[TILE_DOCS];
    __shared__ uint32_t row[MSR_EXPLAIN_MAX_TARGETS];  // first output slot of listed doc j
    __shared__ uint32_t loc[MSR_EXPLAIN_MAX_TARGETS];  // its local ordinal
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    const uint32_t wave = rfl(tid >> 6);
    const uint4 p = a.pairs[blockIdx.x];  // one scalar load
    const uint32_t q = p.x, tile = p.y, n_t = min(p.w, (uint32_t)MSR_EXPLAIN_MAX_TARGETS);

    uint4* const m4 = reinterpret_cast<uint4*>(slot);
    for (uint32_t i = tid; i < (uint32_t)TILE_DOCS / 16u; i += NT) m4[i] = make_uint4(0, 0, 0, 0);
    uint2 it = make_uint2(0, 0);
    if (tid < n_t) it = a.items[p.z + tid];
    __syncthreads();  // the map is zero before a listed doc marks its byte (another thread zeroed it)
    if (tid < n_t) {
        const uint32_t l = min(it.y, (uint32_t)TILE_DOCS - 1u);  // (the host lists local ordinals below the tile size)
        slot[l] = (uint8_t)(tid + 1);
        row[tid] = it.x;
        loc[tid] = l;
    }
    __syncthreads();

    const uint2 qr = a.q_range[q];
    const uint32_t* const seg_row = a.seg_ptr + (uint64_t)tile * (a.n_terms + 1);
    const uint4* const vecs = reinterpret_cast<const uint4*>(a.postings);
    for (uint32_t k = qr.x + wave; k < qr.y; k += NW) {  // (wave-uniform)
        const uint2 en = a.ents[k];
        const uint32_t code = rfl(en.x), j = rfl(en.y);
        if (code & kExplainDense) {
            const uint32_t s = code & 0xFFu;  // dense slot: pair s / 2, low half when even
            if (lane < n_t) {
                const uint32_t v = a.dense[((uint64_t)tile * a.n_pairs + (s >> 1)) * (uint32_t)TILE_DOCS + loc[lane]];
                const uint32_t w = (s & 1u) ? v >> 16 : v & 0xFFFFu;
                if (w != 0) a.out[row[lane] + j] = w;
            }
            continue;
        }
        const uint32_t s0 = seg_row[code], len = seg_row[code + 1] - s0;  // vecs of the segment
        const uint64_t v0 = (uint64_t)s0 - a.vec_base;
        for (uint32_t off = 0; off < len; off += 64 * UL) {
            uint4 x[UL];
#pragma unroll
            for (uint32_t u = 0; u < UL; ++u) {
                const uint32_t v = off + u * 64 + lane;
                x[u] = v < len ? vecs[v0 + v] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (uint32_t u = 0; u < UL; ++u) {
                const uint32_t pp[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t w = pp[e] >> 16;  // unsigned: weights of 32 768 and above keep their value
                    if (w != 0) {                    // padding (weight 0) never reaches the map
                        const uint32_t l = pp[e] & 0xFFFFu;
                        const uint32_t s = l < (uint32_t)TILE_DOCS ? slot[l] : 0u;
                        if (s != 0) a.out[row[s - 1] + j] = w;
                    }
                }
            }
        }
    }
}

}  // namespace msr
