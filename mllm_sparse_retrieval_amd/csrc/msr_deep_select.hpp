// Deep lists (msr_search_deep, msr_dense_search_deep; included by msr_device.hip only): the exact top-k of a row of u32
// keys for k up to MSR_DEEP_KMAX = 16384, far above what the tile selectors hold (CAND <= 1024). The producers are the
// ones the search already has: the accumulator dump of score_tiles (MODE 1, column = doc ordinal) and the key matrix of
// the dense GEMMs (column = row of the index).
//
// deep_select_rows<CAP, NT>   one workgroup per row; the row is re-read out of L2 / Infinity Cache in every pass.
//   1. radix select of the k-th best key theta: up to three histogram passes over 11 / 11 / 10 key bits (LDS atomics,
//      2048 bins). A pass counts the members (key != 0) whose higher bits equal the prefix found so far; the bin that
//      holds the k-th key is found by the waves summing 64 bins each and wave 0 scanning the 32 sums and then the 64
//      bins of the chunk (DPP scans, no serial walk). The first pass also counts the members: a row with at most k of
//      them skips the rest of the select (theta = 0: every member is taken).
//   2. one emit pass in column order: every key > theta, and the first r = k - #{key > theta} columns of the tie class
//      key == theta. Only when the class is not taken whole does the pass need its order: a block of 4 * NT columns at
//      a time, tie counts scanned inside the wave and across the waves through LDS. Survivors go to LDS as composites
//      key << 32 | ~col (one LDS atomic per wave and block hands out their slots).
//   3. bitonic sort of the (at most k) composites in LDS, descending: key descending, lower column first.
//   4. plain stores of every slot of the row's k outputs: no zeroed output buffer, no global atomics.
// Columns >= n are never read (the sparse dump and the GEMM leave stale bytes there): the last, partial vec of a row is
// read element by element.
#pragma once

#include "msr_select.hpp"

namespace msr {

constexpr int kDeepBins = 2048;

struct DeepScratch {
    uint32_t ctot[32];      // keys in each chunk of 64 bins, highest bins first
    uint32_t wtot[2][16];   // tie counts of the waves in the current block of the emit pass (double buffered)
    uint32_t bin, above, cnt, total;  // find_bin's answer
    uint32_t n_out;         // composites written so far
    uint32_t pad[3];
};

template <int CAP>
struct DeepLds {
    static constexpr int kBuf = CAP * 8;
    static constexpr int kHist = kDeepBins * 4;
    static constexpr int kTotal = kBuf + kHist + (int)sizeof(DeepScratch);
};

template <int CAP, int NT>
__global__ __launch_bounds__(NT) void deep_select_rows(const DeepArgs a) {
    using L = DeepLds<CAP>;
    constexpr int NW = NT / 64;
    static_assert(NW <= 16 && (CAP & (CAP - 1)) == 0, "wtot holds 16 waves; the sort pads to a power of two <= CAP");
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    uint64_t* const buf = reinterpret_cast<uint64_t*>(lds);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + L::kBuf);
    DeepScratch& ds = *reinterpret_cast<DeepScratch*>(lds + L::kBuf + L::kHist);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = rfl(tid >> 6);
    const uint32_t row = blockIdx.x;
    const uint32_t n = a.n, k = a.k;
    const uint32_t* const src = a.src + (uint64_t)row * a.ld;
    const uint4* const src4 = reinterpret_cast<const uint4*>(src);
    const uint32_t nv = (n + 3) / 4;  // vecs that hold a valid column

    // keys of columns 4i .. 4i+3; a column >= n is not read and enters as 0 (not a member)
    auto load4 = [&](uint32_t i, uint32_t (&x)[4]) {
        const uint32_t c0 = 4 * i;
        if (i < nv && c0 + 4 <= n) {
            const uint4 v = src4[i];
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) x[e] = (i < nv && c0 + e < n) ? src[c0 + e] : 0u;
        }
    };
    // hist[(key >> shift) & mask] over the members whose bits above `pshift` equal `prefix` (all members: !filtered)
    auto hist_pass = [&](uint32_t shift, uint32_t mask, bool filtered, uint32_t pshift, uint32_t prefix) {
        for (uint32_t i = tid; i < (uint32_t)kDeepBins; i += NT) hist[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < nv; i += NT) {
            uint32_t x[4];
            load4(i, x);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x[e] != 0 && (!filtered || (x[e] >> pshift) == prefix)) atomicAdd(&hist[(x[e] >> shift) & mask], 1u);
        }
        __syncthreads();
    };
    // The bin that holds the want-th key counted from the highest bin: ds.bin, with ds.above keys in higher bins and
    // ds.cnt in the bin itself; ds.total = every key of the histogram (fewer than `want`: bin / above / cnt are 0).
    auto find_bin = [&](uint32_t want) {
        for (uint32_t c = wave; c < 32; c += NW) {
            const uint32_t s = wave_sum_u32(hist[kDeepBins - 1 - (c * 64 + lane)]);
            if (lane == 0) ds.ctot[c] = s;
        }
        __syncthreads();
        if (wave == 0) {
            const uint32_t t = lane < 32 ? ds.ctot[lane] : 0u;
            const uint32_t inc = wave_inclusive_scan_u32(t);
            const uint32_t total = rdl(inc, 63);
            uint32_t bin = 0, above = 0, cnt = 0;
            if (total >= want) {  // (wave-uniform)
                const uint32_t c = rfl((uint32_t)__ffsll((long long)__ballot(inc >= want)) - 1u);  // <= 31
                const uint32_t before = rdl(inc - t, c);
                const uint32_t v = hist[kDeepBins - 1 - (c * 64 + lane)];
                const uint32_t inc2 = wave_inclusive_scan_u32(v) + before;
                const uint32_t j = rfl((uint32_t)__ffsll((long long)__ballot(inc2 >= want)) - 1u);
                bin = kDeepBins - 1 - (c * 64 + j);
                above = rdl(inc2 - v, j);
                cnt = rdl(v, j);
            }
            if (lane == 0) {
                ds.bin = bin;
                ds.above = above;
                ds.cnt = cnt;
                ds.total = total;
            }
        }
        __syncthreads();
    };

    // ---- 1. theta = the k-th best key, r of its `ties` columns are taken. theta = 0: every member is taken.
    if (tid == 0) ds.n_out = 0;
    hist_pass(21, 2047, false, 0, 0);
    find_bin(k);
    const uint32_t members = ds.total;
    uint32_t theta = 0, r = 0, ties = 0;
    if (members > k) {  // (workgroup-uniform)
        uint32_t above = ds.above;
        const uint32_t b1 = ds.bin;
        hist_pass(10, 2047, true, 21, b1);
        find_bin(k - above);
        above += ds.above;
        const uint32_t p2 = (b1 << 11) | ds.bin;
        hist_pass(0, 1023, true, 10, p2);
        find_bin(k - above);
        above += ds.above;
        theta = (p2 << 10) | ds.bin;  // a member's key: never 0
        ties = ds.cnt;
        r = k - above;                // 1 <= r <= ties
    }

    // ---- 2. emit, in column order where the tie class is cut
    const bool ordered = r < ties;
    uint32_t run = 0;  // tie columns of the blocks before this one (the same in every thread)
    const uint32_t n_blk = (nv + NT - 1) / NT;
    for (uint32_t b = 0; b < n_blk; ++b) {
        const uint32_t i = b * NT + tid;
        uint32_t x[4];
        load4(i, x);
        uint32_t tie_at = r;  // index of this thread's first tie column inside the class (past the quota: none taken)
        if (ordered && run < r) {  // (workgroup-uniform)
            uint32_t c = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) c += x[e] == theta ? 1u : 0u;
            const uint32_t inc = wave_inclusive_scan_u32(c);
            if (lane == 63) ds.wtot[b & 1][wave] = inc;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < (uint32_t)NW; ++w) {
                const uint32_t t = ds.wtot[b & 1][w];
                all += t;
                before += w < wave ? t : 0u;
            }
            tie_at = run + before + inc - c;
            run += all;
        }
        bool take[4];
        uint32_t n_take = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            take[e] = x[e] > theta;
            if (theta != 0 && x[e] == theta) {
                take[e] = !ordered || tie_at < r;
                ++tie_at;
            }
            n_take += take[e] ? 1u : 0u;
        }
        const uint32_t inc_t = wave_inclusive_scan_u32(n_take);
        const uint32_t tot = rdl(inc_t, 63);
        uint32_t base = 0;
        if (lane == 0 && tot) base = atomicAdd(&ds.n_out, tot);
        uint32_t pos = rfl(base) + inc_t - n_take;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (take[e]) {
                if (pos < (uint32_t)CAP) buf[pos] = ((uint64_t)x[e] << 32) | (uint32_t)~(4 * i + (uint32_t)e);
                ++pos;
            }
    }
    __syncthreads();
    const uint32_t n_sel = min(min(ds.n_out, k), (uint32_t)CAP);  // = min(k, members)

    // ---- 3. bitonic sort, descending, over the next power of two (empty slots are 0: below every composite)
    if (n_sel > 1) {  // (workgroup-uniform)
        uint32_t P = 2;
        while (P < n_sel) P <<= 1;
        for (uint32_t i = n_sel + tid; i < P; i += NT) buf[i] = 0;
        __syncthreads();
        for (uint32_t size = 2; size <= P; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t i = tid; i < P / 2; i += NT) {
                    const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                    const uint64_t x = buf[lo], y = buf[hi];
                    if ((x < y) == ((lo & size) == 0)) {
                        buf[lo] = y;
                        buf[hi] = x;
                    }
                }
                __syncthreads();
            }
    }

    // ---- 4. the row's k slots
    const uint64_t o = (uint64_t)row * k;
    for (uint32_t i = tid; i < k; i += NT) {
        const uint64_t key = i < n_sel ? buf[i] : 0ull;
        const uint32_t sc = (uint32_t)(key >> 32);
        a.out_idx[o + i] = key ? ~(uint32_t)key : 0xFFFFFFFFu;
        a.out_key[o + i] = sc;
        if (a.out_f32) a.out_f32[o + i] = (float)sc;  // round to nearest even, as the merge kernels
    }
    if (tid == 0) a.out_n[row] = (int32_t)n_sel;
}

}  // namespace msr
