// The filtered-search kernels (msr_filter.hpp) and their launchers, a translation unit of their own: the kernels share
// accumulate_tile / tile_select with score_tiles, and compiled beside it they changed the register allocation of eight of
// its instances (same source, another inlining order). Kept apart, every earlier kernel's code is what it was. The host
// paths (msr_search_filtered in msr_device.hip, msr_dense_search_filtered and msr_hybrid_deep_filtered in msr_hybrid.hip) call
// the launchers.
#include "msr_filter.hpp"

namespace msr {

// score_tiles_filtered (msr_filter.hpp) over the shard-local tiles [t_begin, t_end) for queries [a0.q0, a0.q0 + a0.qn):
// launch_score's grid split and instance choice without the dump instance.
int launch_score_filtered(hipStream_t st, uint32_t tile_docs, uint32_t t_begin, uint32_t t_end, const ScoreArgs& a0,
                                 const FilterArgs& f) {
    if (t_end <= t_begin || a0.qn == 0) return MSR_OK;
    for (uint32_t tl0 = t_begin; tl0 < t_end; tl0 += kMaxGridY) {
        ScoreArgs a = a0;
        a.tl0 = tl0;
        const dim3 grid(a.qn, std::min<uint32_t>(kMaxGridY, t_end - tl0));
        // the instance: light with the 512-key buffer / k <= 512 / the 1024-key buffer, in this order
        const bool known = with_tile_shape(tile_docs, [&](auto s) {
            using S = decltype(s);
            constexpr uint32_t T = S::docs, N = S::threads, UU = S::loads, W = S::waves, WR = S::waves_rest;
            if (a.k <= 512 && a.light && S::light)
                hipLaunchKernelGGL((score_tiles_filtered<T, N, UU, W, 512, S::light>), grid, dim3(N), 0, st, a, f);
            else if (a.k <= 512)
                hipLaunchKernelGGL((score_tiles_filtered<T, N, UU, W, 512>), grid, dim3(N), 0, st, a, f);
            else
                hipLaunchKernelGGL((score_tiles_filtered<T, N, UU, WR, 1024>), grid, dim3(N), 0, st, a, f);
        });
        if (!known) return no_tile_shape(tile_docs);
        HIP_TRY(hipGetLastError());
    }
    return MSR_OK;
}

// select_tiles_filtered (msr_filter.hpp) over every tile of the dense route's key matrix: grid = (query of the pass, tile).
int launch_select_filtered(hipStream_t st, uint32_t tile_docs, const SelectArgs& a, const FilterArgs& f) {
    if (a.n_tiles == 0 || a.qn == 0) return MSR_OK;
    if (a.n_tiles > kMaxGridY || a.tpr != a.n_tiles || f.n_tiles != a.n_tiles) {
        set_error("select_tiles_filtered: %u tiles (tpr %u) outside the grid limit of %u", a.n_tiles, a.tpr, kMaxGridY);
        return MSR_E_RANGE;
    }
    const dim3 grid(a.qn, a.n_tiles);
    const bool known = with_tile_shape(tile_docs, [&](auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL((select_tiles_filtered<S::docs, S::threads, 1024>), grid, dim3(S::threads), 0, st, a, f);
    });
    if (!known) return no_tile_shape(tile_docs);
    HIP_TRY(hipGetLastError());
    return MSR_OK;
}

// score_dump_filtered (msr_filter.hpp) over every tile for queries [a.q0, a.q0 + a.qn): the grid split and the instance
// of launch_score's dump branch (the 1024-key instances' waves; no light instance, as the unfiltered dump has none).
int launch_score_dump_filtered(hipStream_t st, uint32_t tile_docs, uint32_t n_tiles, const ScoreArgs& a0, const FilterArgs& f) {
    if (n_tiles == 0 || a0.qn == 0) return MSR_OK;
    if (a0.dump_add != 0 || !a0.dump || f.n_tiles != n_tiles) {
        set_error("score_dump_filtered: dump_add=%u, %u tiles against the sets' %u", a0.dump_add, n_tiles, f.n_tiles);
        return MSR_E_RANGE;
    }
    for (uint32_t tl0 = 0; tl0 < n_tiles; tl0 += kMaxGridY) {
        ScoreArgs a = a0;
        a.tl0 = tl0;
        const dim3 grid(a.qn, std::min<uint32_t>(kMaxGridY, n_tiles - tl0));
        const bool known = with_tile_shape(tile_docs, [&](auto s) {
            using S = decltype(s);
            hipLaunchKernelGGL((score_dump_filtered<S::docs, S::threads, S::loads, S::waves_rest>), grid, dim3(S::threads), 0,
                               st, a, f);
        });
        if (!known) return no_tile_shape(tile_docs);
        HIP_TRY(hipGetLastError());
    }
    return MSR_OK;
}

// mask_key_rows (msr_filter.hpp) over `rows` key rows of `ld` columns; row r is query q0 + r of the call. The bitmap row
// must cover every vec of a key row.
int launch_mask_key_rows(hipStream_t st, uint32_t* D, uint64_t ld, uint32_t rows, uint32_t q0, const FilterArgs& f) {
    if (rows == 0 || ld == 0) return MSR_OK;
    if (ld % 4 != 0 || ld > (uint64_t)f.stride * 32 || rows > kMaxGridY) {
        set_error("mask_key_rows: rows of %llu columns against doc-set rows of %llu bits, %u rows", (unsigned long long)ld,
                  (unsigned long long)f.stride * 32, rows);
        return MSR_E_RANGE;
    }
    MaskRowsArgs a;
    a.D = D;
    a.ld = ld;
    a.q0 = q0;
    a.f = f;
    hipLaunchKernelGGL(mask_key_rows, dim3((uint32_t)((ld + kMaskRowsCols - 1) / kMaskRowsCols), rows), dim3(kMaskRowsThreads), 0,
                       st, a);
    HIP_TRY(hipGetLastError());
    return MSR_OK;
}

}  // namespace msr
