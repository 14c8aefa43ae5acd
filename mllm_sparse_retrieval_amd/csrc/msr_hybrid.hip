// Hybrid path and encode-side sparsifier: the dense fp16 MFMA scorers (the 256 x 256 kernel lives in msr_gemm_w4.hpp:
// dense_scores_256k; here the 128 x 128 kernel for small grids), the fused per-query kernel of single-tile indexes
// (hybrid_tiles), the reference's min-max fusion for multi-tile indexes (fuse_tiles), the log1p-relu top-k sparsifier
// (sparsify_keys), and their C-ABI entry points.
// Selection and list merging reuse the search path's kernels (launch_select / launch_merge, msr_device.hip).
#include <cmath>

#include "msr_accumulate.hpp"
#include "msr_dense_rank.hpp"
#include "msr_gemm_f32.hpp"
#include "msr_gemm_w4.hpp"
#include "msr_sweep.hpp"
#include "msr_fuse_rows.hpp"

using namespace msr;

// ================================================================================================ dense (hybrid path)
// Flat inner-product search over fp16 passage vectors: the dense half of the reference's hybrid search
// (tevatron FaissFlatSearcher / faiss IndexFlatIP, fp16 storage on GPU: src/search.py:232-237,254-270; queries
// normalised at src/search.py:342, corpus at src/encode.py:301). Scores C[q][d] = sum_k Q[q][k] * P[d][k] on MFMA
// (v_mfma_f32_32x32x16_f16, f32 accumulate), written as order-preserving u32 keys into the accumulator layout of
// select_tiles, so that top-`depth` selection and the tile merge are the SAME kernels as on the sparse path.
namespace msr {


// One workgroup = 4 waves = a 128 (queries) x 128 (docs) block, each wave 64 x 64 = 2 x 2 MFMA tiles of 32 x 32.
// K runs in steps of 32 through a double-buffered LDS stage: 128 rows x 32 halves per operand, row stride 80 B
// (5 sixteen-byte slots: 5r mod 16 is a bijection, so the 16-lane groups of ds_read_b128 hit 16 distinct slots).
// The next K-step's global loads (2 x 16 B per operand per thread) are in flight while the current step's 8 MFMAs run.
// Fragment map of v_mfma_f32_32x32x16_f16: lane (r = l & 31, h = l >> 5) holds elements k = 8h .. 8h+7 of row r of A
// and of column r of B (= row r of P). Q has Mpad rows, P has Npad rows (multiples of 128, zero padded), H % 32 == 0.
constexpr int kGemmRowB = 80;                    // LDS row stride in bytes (64 B of data + 16 B pad)
constexpr int kGemmTileB = 128 * kGemmRowB;      // one operand stage

// raw != 0: the f32 bit patterns are written as they are (hybrid_tiles takes the row as floats) instead of keys
__global__ __launch_bounds__(256) void dense_scores(const _Float16* __restrict__ Q, const _Float16* __restrict__ P,
                                                    uint32_t* __restrict__ out, uint32_t M, uint32_t N, uint32_t H,
                                                    uint64_t ld, uint32_t raw) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][2][kGemmTileB];  // [buffer][A|B]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const uint32_t q_blk = blockIdx.x * 128, d_blk = blockIdx.y * 128;
    if (d_blk >= N) {  // a block of padding docs that select_tiles still reads (its rounds are 4*NT docs wide): keys 0
        for (uint32_t i = tid; i < 128 * 32; i += 256) {
            const uint32_t q = q_blk + i / 32;
            if (q < M) reinterpret_cast<uint4*>(out + (uint64_t)q * ld + d_blk)[i % 32] = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    float16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    // global -> LDS assignment: 512 sixteen-byte segments per operand stage, two per thread (rows s/4, segment s%4)
    const uint32_t s0 = tid, s1 = tid + 256;
    const _Float16* ga0 = Q + (uint64_t)(q_blk + s0 / 4) * H + (s0 % 4) * 8;
    const _Float16* ga1 = Q + (uint64_t)(q_blk + s1 / 4) * H + (s1 % 4) * 8;
    const _Float16* gb0 = P + (uint64_t)(d_blk + s0 / 4) * H + (s0 % 4) * 8;
    const _Float16* gb1 = P + (uint64_t)(d_blk + s1 / 4) * H + (s1 % 4) * 8;
    const uint32_t l0 = (s0 / 4) * kGemmRowB + (s0 % 4) * 16, l1 = (s1 / 4) * kGemmRowB + (s1 % 4) * 16;
    uint4 ra0, ra1, rb0, rb1;
    auto g_load = [&](uint32_t k0) {
        ra0 = *reinterpret_cast<const uint4*>(ga0 + k0);
        ra1 = *reinterpret_cast<const uint4*>(ga1 + k0);
        rb0 = *reinterpret_cast<const uint4*>(gb0 + k0);
        rb1 = *reinterpret_cast<const uint4*>(gb1 + k0);
    };
    auto l_store = [&](int buf) {
        *reinterpret_cast<uint4*>(&stage[buf][0][l0]) = ra0;
        *reinterpret_cast<uint4*>(&stage[buf][0][l1]) = ra1;
        *reinterpret_cast<uint4*>(&stage[buf][1][l0]) = rb0;
        *reinterpret_cast<uint4*>(&stage[buf][1][l1]) = rb1;
    };
    const uint32_t fa = (wm + r) * kGemmRowB + 16 * h, fb = (wn + r) * kGemmRowB + 16 * h;
    g_load(0);
    l_store(0);
    __syncthreads();
    const uint32_t KT = H / 32;
    for (uint32_t kt = 0; kt < KT; ++kt) {
        const int cur = (int)(kt & 1);
        if (kt + 1 < KT) g_load((kt + 1) * 32);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const half8 a0 = *reinterpret_cast<const half8*>(&stage[cur][0][fa + 32 * kk]);
            const half8 a1 = *reinterpret_cast<const half8*>(&stage[cur][0][fa + 32 * kGemmRowB + 32 * kk]);
            const half8 b0 = *reinterpret_cast<const half8*>(&stage[cur][1][fb + 32 * kk]);
            const half8 b1 = *reinterpret_cast<const half8*>(&stage[cur][1][fb + 32 * kGemmRowB + 32 * kk]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (kt + 1 < KT) l_store(cur ^ 1);
        __syncthreads();
    }
    // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t d = d_blk + wn + 32 * j + r;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t q = q_blk + wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (q < M) out[(uint64_t)q * ld + d] = d < N ? (raw ? __float_as_uint(acc[i][j][e]) : f32_to_key(acc[i][j][e])) : 0u;
            }
        }
}


}  // namespace msr

struct msr_dense {
    int device = -1;
    hipStream_t stream = nullptr;
    _Float16* d_P = nullptr;  // [n_pad][h]; fp16 handles
    // f32 handles (msr_dense_open_f32): rows [n_pad][hp] in f32, K zero padded to hp (a multiple of kF32KStep)
    bool f32 = false;
    float* d_P32 = nullptr;
    uint32_t hp = 0;
    uint64_t n = 0;
    uint64_t n_pad = 0;       // multiple of 128 and of tile_docs
    uint32_t h = 0;
    uint32_t tile_docs = 0;
    uint32_t n_tiles = 0;
    // hybrid paths: the same rows in doc-ORDINAL order (P_ord[row2ord[r]] = P[r]), in the handle's precision and row
    // layout ([n_pad][h] fp16 or [n_pad][hp] f32), built on first use and kept while the mapping stays the same
    void* d_P_ord = nullptr;
    std::vector<uint32_t> ord_map;
    bool lds_attr_set = false;  // dense_scores_256k needs the 128 KiB dynamic-LDS opt-in once per device
    // device scratch of the fused hybrid call (query matrix, score rows, result lists), kept between calls and only ever
    // grown: six hipMalloc / hipFree pairs of up to 200 MB cost a call more than its kernels
    enum Slot { S_Q = 0, S_S, S_ORD, S_SF, S_N, S_SELF, S_CS, S_META, S_FLAGS, S_QLIST, S_PART, S_SU, S_USRC, S_USPARSE, S_UDENSE,
                S_URANGE, S_UEXT, S_SW_ORD, S_SW_SF, S_SW_N, S_RANK_IN, S_RANK_OUT, S_DEEP_IDX, S_DEEP_KEY, S_DEEP_N, S_FILTER,
                S_HD_S, S_HD_F, S_HD_SRC, S_HD_SIDX, S_HD_SKEY, S_HD_SN, S_HD_FIDX, S_HD_FKEY, S_HD_FN, S_HD_MEM, S_HD_FSRC, S_COUNT };
    void* scratch[S_COUNT] = {};
    size_t scratch_bytes[S_COUNT] = {};
    uint64_t n_device_allocs = 0;  // hipMalloc calls made on behalf of this handle (steady-state calls make none)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // msr_dense_search's laps, created on first use
    void* take(int slot, size_t bytes) {
        if (scratch_bytes[slot] >= bytes && scratch[slot]) return scratch[slot];
        if (scratch[slot]) (void)hipFree(scratch[slot]);
        scratch[slot] = nullptr;
        scratch_bytes[slot] = 0;
        ++n_device_allocs;
        if (hipMalloc(&scratch[slot], bytes) != hipSuccess) {
            scratch[slot] = nullptr;
            return nullptr;
        }
        scratch_bytes[slot] = bytes;
        return scratch[slot];
    }
};

// The part of msr_dense_open / msr_dense_open_f32 after their argument checks: the device check, a handle with its tile
// geometry and stream, and zeroed device rows (d_P, or d_P32 with K padded to hp) into which `upload(dx)` copies the n
// given rows.
template <class Upload>
static int dense_open(uint64_t n, uint32_t h, bool f32, int device, Upload upload, msr_dense** out) {
    int n_dev = 0;
    if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) {
        set_error("no usable HIP device %d; there is no CPU dense search path", device);
        return MSR_E_NODEVICE;
    }
    msr_dense* dx = new (std::nothrow) msr_dense;
    if (!dx) {
        set_error("out of host memory");
        return MSR_E_NOMEM;
    }
    dx->device = device;
    dx->n = n;
    dx->h = h;
    dx->f32 = f32;
    if (f32) dx->hp = (h + kF32KStep - 1) / kF32KStep * kF32KStep;  // zero columns: exactly neutral in the fmaf chain
    dx->tile_docs = n <= 4096 ? 4096 : 8192;
    dx->n_tiles = (uint32_t)std::max<uint64_t>((n + dx->tile_docs - 1) / dx->tile_docs, 1);
    dx->n_pad = (uint64_t)dx->n_tiles * dx->tile_docs;
    const size_t bytes = (size_t)dx->n_pad * (f32 ? (size_t)dx->hp * 4 : (size_t)h * 2);
    void* rows = nullptr;
    const bool ok = hipSetDevice(device) == hipSuccess &&
                    hipStreamCreateWithFlags(&dx->stream, hipStreamNonBlocking) == hipSuccess &&
                    hipMalloc(&rows, bytes) == hipSuccess;
    if (f32)
        dx->d_P32 = (float*)rows;
    else
        dx->d_P = (_Float16*)rows;
    if (!ok || hipMemset(rows, 0, bytes) != hipSuccess || (n && upload(dx) != hipSuccess)) {
        set_error("device setup of the %sdense index failed (%zu bytes)", f32 ? "f32 " : "", bytes);
        msr_dense_close(dx);
        return MSR_E_HIP;
    }
    *out = dx;
    return MSR_OK;
}

extern "C" {

int msr_dense_open(const uint16_t* p_fp16, uint64_t n, uint32_t h, int device, msr_dense** out) {
    if (!out) {
        set_error("msr_dense_open: null output");
        return MSR_E_INVAL;
    }
    *out = nullptr;
    if ((!p_fp16 && n) || h == 0 || h % 32 != 0 || n >= (1ull << 31)) {
        set_error("msr_dense_open: need fp16 rows with a dimension that is a multiple of 32 (got n=%llu, h=%u)",
                  (unsigned long long)n, h);
        return MSR_E_INVAL;
    }
    return dense_open(n, h, false, device, [&](const msr_dense* dx) {
        return hipMemcpy(dx->d_P, p_fp16, (size_t)n * h * 2, hipMemcpyHostToDevice);
    }, out);
}

int msr_dense_open_f32(const float* p, uint64_t n, uint32_t h, int device, msr_dense** out) {
    if (!out) {
        set_error("msr_dense_open_f32: null output");
        return MSR_E_INVAL;
    }
    *out = nullptr;
    if ((!p && n) || h == 0 || h > (1u << 20) || n >= (1ull << 31)) {
        set_error("msr_dense_open_f32: need f32 rows with 1 <= h <= 2^20 and n < 2^31 (got n=%llu, h=%u)",
                  (unsigned long long)n, h);
        return MSR_E_INVAL;
    }
    return dense_open(n, h, true, device, [&](const msr_dense* dx) {
        return hipMemcpy2D(dx->d_P32, (size_t)dx->hp * 4, p, (size_t)h * 4, (size_t)h * 4, n, hipMemcpyHostToDevice);
    }, out);
}

void msr_dense_close(msr_dense* dx) {
    if (!dx) return;
    (void)hipSetDevice(dx->device);
    if (dx->d_P_ord) (void)hipFree(dx->d_P_ord);
    if (dx->d_P) (void)hipFree(dx->d_P);
    if (dx->d_P32) (void)hipFree(dx->d_P32);
    for (void* p : dx->scratch)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : dx->ev)
        if (e) (void)hipEventDestroy(e);
    if (dx->stream) (void)hipStreamDestroy(dx->stream);
    delete dx;
}

// Row blocks (of 256 queries) per GEMM launch: among the chunk sizes that fit (<= rb_max, <= the batch), the one whose
// grid of row blocks x col_blocks fills its last round of the chip's 256 CUs best (2 x 98 blocks leave a quarter of the
// chip idle, 5 x 98 = 490 fill 1.91 rounds); ties go to the larger chunk.
static uint32_t pick_row_blocks(uint32_t col_blocks, uint64_t rb_max, uint32_t batch_row_blocks) {
    uint32_t best = 1;
    double best_eff = 0;
    for (uint64_t rb = 1; rb <= std::min<uint64_t>(rb_max, std::max<uint32_t>(batch_row_blocks, 1)); ++rb) {
        const uint64_t blocks = rb * std::max<uint32_t>(col_blocks, 1);
        const double eff = (double)blocks / (double)((blocks + 255) / 256 * 256);
        if (eff >= best_eff - 1e-9) best_eff = eff, best = (uint32_t)rb;
    }
    return best;
}

// C = Q * P^T as order-preserving keys into out[q][ld] for doc columns [0, n_cover); rows of Q padded to qn_pad (a
// multiple of 256), P rows readable up to n_cover. Doc blocks are launched in slices of at most 65535 (grid y limit).
static int launch_dense_gemm(msr_dense* dx, const _Float16* P, const _Float16* d_Q, uint32_t* d_S, uint32_t qn,
                             uint32_t qn_pad, uint64_t n_cover, uint64_t ld, hipStream_t st, bool force_256 = false,
                             bool raw = false) {
    const bool big = dx->h % 64 == 0 && n_cover % 256 == 0 &&
                     (force_256 || (uint64_t)(qn_pad / 256) * (n_cover / 256) >= 256);
    if (big && !dx->lds_attr_set) {  // 128 KiB of dynamic LDS needs the opt-in (per device: kept in the handle)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(dense_scores_256k<0>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kGkStage));
        dx->lds_attr_set = true;
    }
    const uint64_t blk = big ? 256 : 128;
    for (uint64_t d0 = 0; d0 < n_cover; d0 += blk * kMaxGridY) {
        const uint64_t nd = std::min<uint64_t>(n_cover - d0, blk * kMaxGridY);
        const uint32_t n_left = dx->n > d0 ? (uint32_t)std::min<uint64_t>(dx->n - d0, 0xFFFFFFFFull) : 0u;
        if (big) {
            const uint32_t qb_n = qn_pad / 256, db_n = (uint32_t)(nd / 256);
            hipLaunchKernelGGL(dense_scores_256k<0>, dim3((qb_n * db_n + 7) / 8 * 8), dim3(256), 2 * kGkStage, st, d_Q,
                               P + d0 * dx->h, d_S + d0, qn, n_left, dx->h, ld, qb_n, db_n, raw ? 1u : 0u);
        } else {
            hipLaunchKernelGGL(dense_scores, dim3(qn_pad / 128, (uint32_t)(nd / 128)), dim3(256), 0, st, d_Q, P + d0 * dx->h,
                               d_S + d0, qn, n_left, dx->h, ld, raw ? 1u : 0u);
        }
        HIP_TRY(hipGetLastError());
    }
    return MSR_OK;
}

// The f32 GEMM of an f32 handle: keys (raw: f32 bit patterns) of C = Q * P^T into out[q][ld] for doc columns
// [0, n_cover); P is [>= n_cover][dx->hp] (d_P32 or the ordinal-ordered copy), Q rows padded to qn_pad (a multiple of
// 128) and K to dx->hp in the device copy. Doc blocks in slices of at most 65535 (grid y limit).
static int launch_dense_gemm_f32(msr_dense* dx, const float* P, const float* d_Q, uint32_t* d_S, uint32_t qn,
                                 uint32_t qn_pad, uint64_t n_cover, uint64_t ld, hipStream_t st, bool raw = false) {
    for (uint64_t d0 = 0; d0 < n_cover; d0 += 128ull * kMaxGridY) {
        const uint64_t nd = std::min<uint64_t>(n_cover - d0, 128ull * kMaxGridY);
        const uint32_t n_left = dx->n > d0 ? (uint32_t)std::min<uint64_t>(dx->n - d0, 0xFFFFFFFFull) : 0u;
        const dim3 grid(qn_pad / 128, (uint32_t)(nd / 128));
        if (raw)
            hipLaunchKernelGGL(dense_scores_f32<1>, grid, dim3(256), 0, st, d_Q, P + d0 * dx->hp, d_S + d0, qn, n_left,
                               dx->hp, ld);
        else
            hipLaunchKernelGGL(dense_scores_f32<0>, grid, dim3(256), 0, st, d_Q, P + d0 * dx->hp, d_S + d0, qn, n_left,
                               dx->hp, ld);
        HIP_TRY(hipGetLastError());
    }
    return MSR_OK;
}

// The passes of one dense call over `nq` queries, shared by the search and by msr_dense_rank_rows (so both walk the same
// passes with the same GEMM instances): queries per pass, the device query copy's row size and the doc columns scored.
struct DensePasses {
    uint32_t qt_pad;   // rows of d_Q / d_S per pass (a multiple of 256)
    uint32_t qt;       // queries per pass
    size_t q_row;      // bytes per row of the device query copy
    uint64_t n_cover;  // the GEMM writes doc columns [0, n_cover) of every score row; [n_cover, n_pad) are never written
};

static DensePasses dense_passes(const msr_dense* dx, int nq) {
    DensePasses ps;
    // queries per pass: score rows of at most ~256 MB (they are read back by select_tiles out of the Infinity Cache, and
    // the buffer stays with the handle), the GEMM grid filling its last round of 256 CUs as well as it can
    const uint32_t nq_pad_all = (uint32_t)((std::max(nq, 1) + 255) / 256 * 256);
    const uint64_t rb_max = std::max<uint64_t>(1, (256ull << 20) / (std::max<uint64_t>(dx->n_pad, 256) * 4 * 256));
    ps.qt_pad = 256u * pick_row_blocks((uint32_t)(std::max<uint64_t>(dx->n_pad, 256) / 256), rb_max, nq_pad_all / 256);
    ps.qt = (uint32_t)std::min<uint32_t>(ps.qt_pad, std::max(nq, 1));
    ps.q_row = dx->f32 ? (size_t)dx->hp * 4 : (size_t)dx->h * 2;
    // doc blocks: up to the end of the last select round that holds a real doc (a round = 4 docs x threads of
    // the select instance: 1024 docs at 4096-doc tiles, 2048 at 8192); padding beyond that is never read
    const uint64_t round_docs = dx->tile_docs == 4096 ? 1024 : 2048;
    ps.n_cover = std::min<uint64_t>(dx->n_pad, (dx->n + round_docs - 1) / round_docs * round_docs);
    return ps;
}

// One pass: queries [q0, q0 + qn) of q_host into d_Q (rows zero padded to a multiple of 256, K to the handle's row size)
// and their keys into d_S[q][n_pad], all on dx->stream. e0 is recorded before the upload (time_upload) or after it.
static int dense_pass_scores(msr_dense* dx, const DensePasses& ps, const void* q_host, int q0, uint32_t qn, uint8_t* d_Q,
                             uint32_t* d_S, hipEvent_t e0, bool time_upload, const char* who) {
    const uint32_t qn_pad = (qn + 255) / 256 * 256;
    // f32 rows land in a K-padded copy (zero columns are neutral in the fmaf chain), fp16 rows as they are
    const size_t h_row = (size_t)dx->h * (dx->f32 ? 4 : 2);
    const bool c = (!time_upload || hipEventRecord(e0, dx->stream) == hipSuccess) &&
                   hipMemsetAsync(d_Q, 0, (size_t)qn_pad * ps.q_row, dx->stream) == hipSuccess &&
                   (ps.q_row == h_row
                        ? hipMemcpyAsync(d_Q, (const uint8_t*)q_host + (size_t)q0 * h_row, (size_t)qn * h_row,
                                         hipMemcpyHostToDevice, dx->stream)
                        : hipMemcpy2DAsync(d_Q, ps.q_row, (const uint8_t*)q_host + (size_t)q0 * h_row, h_row, h_row, qn,
                                           hipMemcpyHostToDevice, dx->stream)) == hipSuccess &&
                   (time_upload || hipEventRecord(e0, dx->stream) == hipSuccess);
    if (!c) {
        set_error("query upload failed in %s", who);
        return MSR_E_HIP;
    }
    return dx->f32 ? launch_dense_gemm_f32(dx, dx->d_P32, (const float*)d_Q, d_S, qn, qn_pad, ps.n_cover, dx->n_pad, dx->stream)
                   : launch_dense_gemm(dx, dx->d_P, (const _Float16*)d_Q, d_S, qn, qn_pad, ps.n_cover, dx->n_pad, dx->stream);
}

}  // extern "C"

// The pass loop of every dense call: queries go through the GEMM `ps.qt` at a time, and per pass the caller's `stage`
// turns the pass's key rows into its result, which its `fetch` copies back. Use: begin() (device, passes, the query and
// score scratch), the caller's own scratch slots, ready(), run().
struct DensePassLoop {
    msr_dense* dx;
    const char* who;           // the call, as its error messages name it
    bool time_upload = true;   // e0 before the query upload (false: after it, msr_dense_search's gemm_ms)
    const char* failed = nullptr;  // subject of the failure message when it is not "<who>:"
    DensePasses ps{};
    uint8_t* d_Q = nullptr;
    uint32_t* d_S = nullptr;
    DensePassLoop(msr_dense* handle, const char* name) : dx(handle), who(name) {}

    int begin(int nq) {
        HIP_TRY(hipSetDevice(dx->device));
        ps = dense_passes(dx, nq);
        // device scratch and events live on the handle (only ever grown): at the reference's --batch_size 2
        // (scripts/search.sh:29) seven hipMalloc / hipFree pairs per call cost more than the search
        d_Q = (uint8_t*)dx->take(msr_dense::S_Q, (size_t)ps.qt_pad * ps.q_row);
        d_S = (uint32_t*)dx->take(msr_dense::S_S, (size_t)ps.qt_pad * dx->n_pad * 4);
        return MSR_OK;
    }
    // `own`: the caller got its own slots. False: something is missing (the caller reports it, MSR_E_NOMEM).
    bool ready(bool own) {
        bool ok = d_Q && d_S && own;
        for (hipEvent_t& e : dx->ev)
            if (ok && !e) ok = hipEventCreate(&e) == hipSuccess;
        return ok;
    }
    // prologue(q0, qn, &skip) -> rc runs before the pass's upload and may skip the pass, GEMM included;
    // stage(q0, qn, d_S) -> rc enqueues the pass's kernels; fetch(q0, qn) -> bool enqueues its copies back.
    // ms0 / ms1 (may be null): GEMM and stage milliseconds, summed over the passes.
    template <class Prologue, class Stage, class Fetch>
    int run(const void* q_host, int nq, float* ms0, float* ms1, Prologue prologue, Stage stage, Fetch fetch) {
        hipEvent_t e0 = dx->ev[0], e1 = dx->ev[1], e2 = dx->ev[2];
        const int qt = (int)ps.qt;
        double t_gemm = 0, t_stage = 0;
        int rc = MSR_OK;
        for (int q0 = 0; q0 < nq && rc == MSR_OK; q0 += qt) {
            const uint32_t qn = (uint32_t)std::min(qt, nq - q0);
            bool skip = false;
            rc = prologue(q0, qn, &skip);
            if (rc != MSR_OK || skip) continue;
            rc = dense_pass_scores(dx, ps, q_host, q0, qn, d_Q, d_S, e0, time_upload, who);
            if (rc != MSR_OK) break;
            (void)hipEventRecord(e1, dx->stream);
            rc = stage(q0, qn, d_S);
            if (rc != MSR_OK) break;
            (void)hipEventRecord(e2, dx->stream);
            if (!fetch(q0, qn) || hipStreamSynchronize(dx->stream) != hipSuccess) {
                set_error("%s%s kernels or result download failed: %s", failed ? failed : who, failed ? "" : ":",
                          hipGetErrorString(hipGetLastError()));
                rc = MSR_E_HIP;
                break;
            }
            float a = 0, b = 0;
            (void)hipEventElapsedTime(&a, e0, e1);
            (void)hipEventElapsedTime(&b, e1, e2);
            t_gemm += a;
            t_stage += b;
        }
        if (ms0) *ms0 = (float)t_gemm;
        if (ms1) *ms1 = (float)t_stage;
        return rc;
    }
    template <class Stage, class Fetch>
    int run(const void* q_host, int nq, float* ms0, float* ms1, Stage stage, Fetch fetch) {
        return run(q_host, nq, ms0, ms1, [](int, uint32_t, bool*) { return (int)MSR_OK; }, stage, fetch);
    }
};

// The per-tile lists and the result rows of a pass of the plain and the filtered search, on the handle's slots: take(),
// then per pass stage() (select_tiles, or select_tiles_filtered with the call's doc sets, then the merge) and fetch().
struct DenseLists {
    msr_dense* dx;
    int k;
    uint64_t* d_part = nullptr;
    uint32_t *d_ord = nullptr, *d_su = nullptr;
    float* d_sf = nullptr;
    int32_t* d_n = nullptr;
    bool take(uint32_t qt) {
        const size_t perq = (size_t)qt * k;
        d_part = (uint64_t*)dx->take(msr_dense::S_PART, (size_t)dx->n_tiles * perq * 8);
        d_ord = (uint32_t*)dx->take(msr_dense::S_ORD, perq * 4);
        d_su = (uint32_t*)dx->take(msr_dense::S_SU, perq * 4);
        d_sf = (float*)dx->take(msr_dense::S_SF, perq * 4);
        d_n = (int32_t*)dx->take(msr_dense::S_N, (size_t)qt * 4);
        return d_part && d_ord && d_su && d_sf && d_n;
    }
    // fa = null: launch_select, with `unsorted` on a one-tile handle (the fusion takes the list as a set)
    int stage(int q0, uint32_t qn, const uint32_t* d_S, bool unsorted, const FilterArgs* fa) const {
        SelectArgs se;
        se.src = d_S;
        se.part = d_part;
        se.n_docs = dx->n;
        se.n_tiles = dx->n_tiles;
        se.tpr = dx->n_tiles;
        se.rank = 0;
        se.nq = qn;
        se.q0 = fa ? (uint32_t)q0 : 0u;  // filtered: the pass's first query in the call (q_set is indexed by q0 + qi, `part` by qi)
        se.qn = qn;
        se.k = (uint32_t)k;
        se.unsorted = (unsorted && dx->n_tiles == 1) ? 1u : 0u;
        int rc = fa ? launch_select_filtered(dx->stream, dx->tile_docs, se, *fa) : launch_select(dx->stream, dx->tile_docs, se);
        if (rc != MSR_OK) return rc;
        MergeArgs ma;
        ma.lists = d_part;
        ma.list_stride = (uint64_t)qn * k;
        ma.n_lists = dx->n_tiles;
        ma.nq = qn;
        ma.k = (uint32_t)k;
        ma.out_keys = nullptr;
        ma.out_ord = d_ord;
        ma.out_score_u32 = d_su;
        ma.out_score = d_sf;
        ma.out_n = d_n;
        return launch_merge(dx->stream, ma);
    }
    bool fetch(int q0, uint32_t qn, uint32_t* out_idx, uint32_t* out_key, int32_t* out_n, hipMemcpyKind kind) const {
        return hipMemcpyAsync(out_idx + (size_t)q0 * k, d_ord, (size_t)qn * k * 4, kind, dx->stream) == hipSuccess &&
               hipMemcpyAsync(out_key + (size_t)q0 * k, d_su, (size_t)qn * k * 4, kind, dx->stream) == hipSuccess &&
               hipMemcpyAsync(out_n + q0, d_n, (size_t)qn * 4, kind, dx->stream) == hipSuccess;
    }
};

// The refusal of queries in the other precision than the handle's rows
static int dense_precision_check(const char* who, const msr_dense* dx, int q_is_f32) {
    if ((q_is_f32 != 0) == dx->f32) return MSR_OK;
    if (dx->f32)
        set_error("%s: q_is_f32 = 0 but the dense handle holds f32 rows (msr_dense_open_f32); pass f32 queries with "
                  "q_is_f32 = 1, or open an fp16 handle with msr_dense_open", who);
    else
        set_error("%s: q_is_f32 = 1 but the dense handle holds fp16 rows (msr_dense_open); pass fp16 queries with "
                  "q_is_f32 = 0, or open an f32 handle with msr_dense_open_f32", who);
    return MSR_E_INVAL;
}

// ... and of a handle without a device
static int dense_device_check(const char* who, const msr_dense* dx) {
    if (dx->device >= 0) return MSR_OK;
    set_error("%s: the dense handle has no HIP device; there is no CPU dense search path", who);
    return MSR_E_NODEVICE;
}

// to_device = true: out_* are DEVICE buffers ([nq][k] / [nq]) filled on dx->stream (hybrid path); else host buffers.
// q: [nq][h] fp16 (uint16_t) or, on an f32 handle, f32 rows. gemm_ms starts after the query upload.
static int dense_search_impl(msr_dense* dx, const void* q_host, int nq, int k, uint32_t* out_idx, uint32_t* out_key,
                             int32_t* out_n, float* gemm_ms, float* select_ms, bool to_device, bool unsorted = false) {
    if (!dx || nq < 0 || (nq && !q_host) || !out_idx || !out_key || !out_n) {
        set_error("msr_dense_search: bad argument");
        return MSR_E_INVAL;
    }
    if (k < 1 || k > MSR_KMAX) {
        set_error("k must be in [1, %d] (got %d)", MSR_KMAX, k);
        return MSR_E_RANGE;
    }
    DensePassLoop lp(dx, "msr_dense_search");
    lp.time_upload = false;
    lp.failed = "dense search";
    if (int rc = lp.begin(nq)) return rc;
    DenseLists ls{dx, k};
    if (!lp.ready(ls.take(lp.ps.qt))) {
        set_error("device allocation failed in msr_dense_search (%u queries per pass x %llu docs)", lp.ps.qt, (unsigned long long)dx->n_pad);
        if (gemm_ms) *gemm_ms = 0.f;
        if (select_ms) *select_ms = 0.f;
        return MSR_E_NOMEM;
    }
    const hipMemcpyKind kind = to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    return lp.run(q_host, nq, gemm_ms, select_ms,
                  [&](int q0, uint32_t qn, const uint32_t* d_S) { return ls.stage(q0, qn, d_S, unsorted, nullptr); },
                  [&](int q0, uint32_t qn) { return ls.fetch(q0, qn, out_idx, out_key, out_n, kind); });
}

extern "C" {

int msr_dense_stats(const msr_dense* dx, uint64_t out[4]) {
    if (!dx || !out) {
        set_error("msr_dense_stats: bad argument");
        return MSR_E_INVAL;
    }
    uint64_t bytes = 0;
    for (size_t b : dx->scratch_bytes) bytes += b;
    out[0] = dx->n_device_allocs;
    out[1] = bytes;
    out[2] = dx->n;
    out[3] = dx->h;
    return MSR_OK;
}

int msr_dense_search(msr_dense* dx, const uint16_t* q_fp16, int nq, int k, uint32_t* out_idx, uint32_t* out_key,
                     int32_t* out_n, float* gemm_ms, float* select_ms) {
    if (dx && dx->f32) {
        set_error("msr_dense_search: this handle holds f32 rows (msr_dense_open_f32); search it with msr_dense_search_f32");
        return MSR_E_INVAL;
    }
    return dense_search_impl(dx, q_fp16, nq, k, out_idx, out_key, out_n, gemm_ms, select_ms, false);
}

int msr_dense_search_f32(msr_dense* dx, const float* q, int nq, int k, uint32_t* out_idx, uint32_t* out_key,
                         int32_t* out_n, float* gemm_ms, float* select_ms) {
    if (dx && !dx->f32) {
        set_error("msr_dense_search_f32: this handle holds fp16 rows (msr_dense_open); search it with msr_dense_search");
        return MSR_E_INVAL;
    }
    return dense_search_impl(dx, q, nq, k, out_idx, out_key, out_n, gemm_ms, select_ms, false);
}

// Exact ranks of listed rows: the pass loop and the GEMM of the search (DensePassLoop), then ONE count
// kernel per pass over the score rows (msr_dense_rank.hpp) in the place of select + merge. Per pass one upload
// {t_ptr rebased to the pass | self | the pass's slice of t_row} and the ranks and keys of its entries back.
int msr_dense_rank_rows(msr_dense* dx, const void* q, int q_is_f32, int nq, const int64_t* t_ptr, const uint32_t* t_row,
                        const int32_t* self_row, uint32_t* out_rank, uint32_t* out_key, float ms[2]) {
    const char* const who = "msr_dense_rank_rows";
    // ---- checks, all before any device work
    if (!dx || !t_ptr || nq < 0 || (nq && !q)) {
        set_error("%s: bad argument", who);
        return MSR_E_INVAL;
    }
    if (t_ptr[0] != 0) {
        set_error("%s: t_ptr must start at 0 (got %lld)", who, (long long)t_ptr[0]);
        return MSR_E_INVAL;
    }
    for (int i = 0; i < nq; ++i)
        if (t_ptr[i + 1] < t_ptr[i]) {
            set_error("%s: t_ptr decreases at query %d", who, i);
            return MSR_E_INVAL;
        }
    const int64_t n_ent = t_ptr[nq];
    if (n_ent && (!t_row || !out_rank || !out_key)) {
        set_error("%s: null t_row / out_rank / out_key with %lld listed rows", who, (long long)n_ent);
        return MSR_E_INVAL;
    }
    if (int rc0 = dense_precision_check(who, dx, q_is_f32)) return rc0;
    for (int i = 0; i < nq; ++i) {
        if (t_ptr[i + 1] - t_ptr[i] > MSR_DENSE_RANK_MAX_TARGETS) {
            set_error("%s: query %d lists %lld rows, at most MSR_DENSE_RANK_MAX_TARGETS = %d", who, i,
                      (long long)(t_ptr[i + 1] - t_ptr[i]), MSR_DENSE_RANK_MAX_TARGETS);
            return MSR_E_RANGE;
        }
        if (self_row && self_row[i] >= 0 && (uint64_t)self_row[i] >= dx->n) {
            set_error("%s: self_row[%d] = %d, the index holds %llu rows", who, i, self_row[i], (unsigned long long)dx->n);
            return MSR_E_RANGE;
        }
    }
    for (int64_t e = 0; e < n_ent; ++e)
        if (t_row[e] >= dx->n) {
            set_error("%s: listed row %u at entry %lld, the index holds %llu rows", who, t_row[e], (long long)e,
                      (unsigned long long)dx->n);
            return MSR_E_RANGE;
        }
    if (ms) ms[0] = ms[1] = 0.f;
    if (nq == 0 || n_ent == 0) return MSR_OK;
    // ---- scratch of the largest pass
    DensePassLoop lp(dx, who);
    if (int rc = lp.begin(nq)) return rc;
    const int qt = (int)lp.ps.qt;
    int64_t max_pe = 0;
    for (int q0 = 0; q0 < nq; q0 += qt) max_pe = std::max<int64_t>(max_pe, t_ptr[std::min(nq, q0 + qt)] - t_ptr[q0]);
    uint32_t* d_in = (uint32_t*)dx->take(msr_dense::S_RANK_IN, ((size_t)2 * qt + 1 + (size_t)max_pe) * 4);
    uint32_t* d_out = (uint32_t*)dx->take(msr_dense::S_RANK_OUT, (size_t)2 * max_pe * 4);
    if (!lp.ready(d_in && d_out)) {
        set_error("device allocation failed in %s (%d queries per pass x %llu docs)", who, qt, (unsigned long long)dx->n_pad);
        return MSR_E_NOMEM;
    }
    std::vector<uint32_t> in;  // host image of the pass's upload
    uint32_t pe = 0, t_max = 0;  // the pass's entries, and the most one of its queries lists
    return lp.run(
        q, nq, ms, ms ? ms + 1 : nullptr,
        [&](int q0, uint32_t qn, bool* skip) {
            const int64_t ent0 = t_ptr[q0];
            pe = (uint32_t)(t_ptr[q0 + qn] - ent0);
            if ((*skip = pe == 0)) return (int)MSR_OK;  // nothing listed in this pass: no GEMM either
            in.assign((size_t)2 * qn + 1 + pe, 0u);
            t_max = 0;
            for (uint32_t i = 0; i <= qn; ++i) in[i] = (uint32_t)(t_ptr[q0 + i] - ent0);
            for (uint32_t i = 0; i < qn; ++i) {
                in[qn + 1 + i] = (uint32_t)(self_row ? std::max<int32_t>(self_row[q0 + i], -1) : -1);
                t_max = std::max(t_max, in[i + 1] - in[i]);
            }
            std::copy(t_row + ent0, t_row + ent0 + pe, in.begin() + 2 * qn + 1);
            if (hipMemcpyAsync(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice, dx->stream) != hipSuccess) {
                set_error("%s: upload of the listed rows failed", who);
                return (int)MSR_E_HIP;
            }
            return (int)MSR_OK;
        },
        [&](int, uint32_t qn, const uint32_t* d_S) {
            DenseRankArgs ra;
            ra.S = d_S;
            ra.ld = dx->n_pad;
            ra.n = (uint32_t)dx->n;
            ra.t_ptr = d_in;
            ra.self_row = reinterpret_cast<const int32_t*>(d_in + qn + 1);
            ra.t_row = d_in + 2 * qn + 1;
            ra.out_rank = d_out;
            ra.out_key = d_out + pe;
            hipLaunchKernelGGL(dense_rank_rows, dim3(qn, (t_max + kDenseRankGroup - 1) / kDenseRankGroup), dim3(kDenseRankThreads), 0,
                               dx->stream, ra);
            HIP_TRY(hipGetLastError());
            return (int)MSR_OK;
        },
        [&](int q0, uint32_t) {
            const int64_t ent0 = t_ptr[q0];
            return hipMemcpyAsync(out_rank + ent0, d_out, (size_t)pe * 4, hipMemcpyDeviceToHost, dx->stream) == hipSuccess &&
                   hipMemcpyAsync(out_key + ent0, d_out + pe, (size_t)pe * 4, hipMemcpyDeviceToHost, dx->stream) == hipSuccess;
        });
}

// Deep lists on the dense route: the pass loop and the GEMM of the search (DensePassLoop), then
// deep_select_rows (msr_deep_select.hpp, launched through msr_device.hip) over the pass's key rows in the place of
// select_tiles + merge_lists, for k up to MSR_DEEP_KMAX.
int msr_dense_search_deep(msr_dense* dx, const void* q, int q_is_f32, int nq, int k, uint32_t* out_idx, uint32_t* out_key,
                          int32_t* out_n, float ms[2]) {
    const char* const who = "msr_dense_search_deep";
    if (!dx || nq < 0 || (nq && !q) || !out_idx || !out_key || !out_n) {
        set_error("%s: bad argument", who);
        return MSR_E_INVAL;
    }
    if (int rc0 = dense_precision_check(who, dx, q_is_f32)) return rc0;
    if (k < 1 || k > MSR_DEEP_KMAX) {
        set_error("%s: k must be in [1, MSR_DEEP_KMAX = %d] (got %d)", who, MSR_DEEP_KMAX, k);
        return MSR_E_RANGE;
    }
    if (int rc0 = dense_device_check(who, dx)) return rc0;
    if (ms) ms[0] = ms[1] = 0.f;
    if (nq == 0) return MSR_OK;
    DensePassLoop lp(dx, who);
    if (int rc = lp.begin(nq)) return rc;
    const uint32_t qt = lp.ps.qt;
    const size_t perq = (size_t)qt * k;
    uint32_t* d_idx = (uint32_t*)dx->take(msr_dense::S_DEEP_IDX, perq * 4);
    uint32_t* d_key = (uint32_t*)dx->take(msr_dense::S_DEEP_KEY, perq * 4);
    int32_t* d_n = (int32_t*)dx->take(msr_dense::S_DEEP_N, (size_t)qt * 4);
    if (!lp.ready(d_idx && d_key && d_n)) {
        set_error("device allocation failed in %s (%u queries per pass x %llu docs, k = %d)", who, qt, (unsigned long long)dx->n_pad, k);
        return MSR_E_NOMEM;
    }
    return lp.run(
        q, nq, ms, ms ? ms + 1 : nullptr,
        [&](int, uint32_t qn, const uint32_t* d_S) {
            DeepArgs da;
            da.src = d_S;
            da.ld = dx->n_pad;
            da.n = (uint32_t)dx->n;
            da.rows = qn;
            da.k = (uint32_t)k;
            da.out_idx = d_idx;
            da.out_key = d_key;
            da.out_f32 = nullptr;
            da.out_n = d_n;
            return launch_deep_select(dx->stream, da);
        },
        [&](int q0, uint32_t qn) {
            return hipMemcpyAsync(out_idx + (size_t)q0 * k, d_idx, (size_t)qn * k * 4, hipMemcpyDeviceToHost, dx->stream) == hipSuccess &&
                   hipMemcpyAsync(out_key + (size_t)q0 * k, d_key, (size_t)qn * k * 4, hipMemcpyDeviceToHost, dx->stream) == hipSuccess &&
                   hipMemcpyAsync(out_n + q0, d_n, (size_t)qn * 4, hipMemcpyDeviceToHost, dx->stream) == hipSuccess;
        });
}

// Filtered search on the dense route: the pass loop and the GEMM of the search (DensePassLoop), then
// select_tiles_filtered (msr_filter.hpp, launched through msr_filter.hip) in the place of select_tiles, then the search's
// merge. The doc sets are uploaded once per call (S_FILTER: bitmap | any | q_set); the kernel indexes q_set by the call's
// query, the per-tile lists are pass-local.
int msr_dense_search_filtered(msr_dense* dx, const void* q, int q_is_f32, int nq, int k, const uint32_t* set_bits,
                              int n_sets, const int32_t* q_set, uint32_t* out_idx, uint32_t* out_key, int32_t* out_n,
                              float ms[2]) {
    const char* const who = "msr_dense_search_filtered";
    if (!dx || nq < 0 || (nq && !q) || !out_idx || !out_key || !out_n) {
        set_error("%s: bad argument", who);
        return MSR_E_INVAL;
    }
    if (int rc0 = filter_check_shapes(who, set_bits, n_sets, q_set)) return rc0;
    if (int rc0 = dense_precision_check(who, dx, q_is_f32)) return rc0;
    if (k < 1 || k > MSR_KMAX) {
        set_error("%s: k must be in [1, MSR_KMAX = %d] (got %d)", who, MSR_KMAX, k);
        return MSR_E_RANGE;
    }
    if (int rc0 = filter_check_ranges(who, n_sets, q_set, nq)) return rc0;
    if (int rc0 = dense_device_check(who, dx)) return rc0;
    if (ms) ms[0] = ms[1] = 0.f;
    if (nq == 0) return MSR_OK;
    DensePassLoop lp(dx, who);
    if (int rc = lp.begin(nq)) return rc;
    FilterImage fi;
    fi.build(set_bits, n_sets, q_set, nq, dx->n, dx->tile_docs, dx->n_tiles);
    auto al = [](size_t n) { return (n + 63) / 64 * 64; };  // sub-buffers start on 256-byte boundaries (in u32 units)
    const size_t o_bits = 0, o_any = al(fi.bits.size()), o_qs = o_any + al(fi.any.size()), f_words = o_qs + al(fi.q_set.size());
    DenseLists ls{dx, k};
    const bool own = ls.take(lp.ps.qt);
    uint32_t* d_f = (uint32_t*)dx->take(msr_dense::S_FILTER, f_words * 4);
    if (!lp.ready(own && d_f)) {
        set_error("device allocation failed in %s (%u queries per pass x %llu docs, %d sets)", who, lp.ps.qt,
                  (unsigned long long)dx->n_pad, n_sets);
        return MSR_E_NOMEM;
    }
    if (hipMemcpy(d_f + o_bits, fi.bits.data(), fi.bits.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_f + o_any, fi.any.data(), fi.any.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_f + o_qs, fi.q_set.data(), fi.q_set.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: upload of the doc sets failed", who);
        return MSR_E_HIP;
    }
    FilterArgs fa;
    fa.bits = d_f + o_bits;
    fa.any = reinterpret_cast<const uint8_t*>(d_f + o_any);
    fa.q_set = reinterpret_cast<const int32_t*>(d_f + o_qs);
    fa.stride = fi.stride;
    fa.n_tiles = dx->n_tiles;
    return lp.run(q, nq, ms, ms ? ms + 1 : nullptr,
                  [&](int q0, uint32_t qn, const uint32_t* d_S) { return ls.stage(q0, qn, d_S, false, &fa); },
                  [&](int q0, uint32_t qn) { return ls.fetch(q0, qn, out_idx, out_key, out_n, hipMemcpyDeviceToHost); });
}

}  // extern "C"

// ================================================================================================ hybrid fusion
// The reference's fuse() (src/hybrid.py:32-53) on the GPU: per query, over the union of the dense and the sparse
// top-`depth` lists,  fused(doc) = w_dense * (d - min_d) / max(max_d - min_d, 1e-9)   [if the dense list holds doc]
//                                + w_sparse * (s - min_s) / max(max_s - min_s, 1e-9)  [if the sparse list holds doc]
// with min/max over each UNFILTERED list (get_run_dict, src/search.py:76-81) and the query's own doc skipped when
// remove_query is set (src/search.py:72-74). Fused scores are built in an LDS accumulator tile over doc ordinals and
// the best k are selected by the same tile_select as everywhere else. f32 arithmetic (the reference mixes f32 and
// f64 depending on the numpy version): scores agree within the north star's 1e-5. The f32 operation sequence is the
// one of the contract in include/msr.h (msr_hybrid_search) — the quotient as a multiplication by the reciprocal, exactly
// 1 at the maximum, two fused adds — so this path returns the score bits of hybrid_tiles and hybrid_fuse_query.
namespace msr {

struct FuseArgs {
    const uint64_t* s_keys;   // [nq][depth] sparse keys (score<<32 | ~ordinal), best first, 0 padded
    const uint32_t* d_idx;    // [nq][depth] dense row indices, best first
    const uint32_t* d_key;    // [nq][depth] order-preserving keys of the dense f32 scores, 0 padded
    const int32_t* d_n;       // [nq]
    const uint32_t* row2ord;  // dense row -> sparse doc ordinal
    const int32_t* self_ord;  // [nq] ordinal to skip (remove_query) or -1; may be null
    uint64_t* part;           // [n_tiles][nq][k]
    uint64_t n_docs;
    uint32_t nq, depth, k;
    float w_dense, w_sparse;
};


template <int TILE_DOCS, int NT, int CAND>
__global__ __launch_bounds__(NT) void fuse_tiles(const FuseArgs a) {
    using L = TileLds<TILE_DOCS, NT, CAND>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    __shared__ uint8_t member[TILE_DOCS];
    uint32_t* const acc = reinterpret_cast<uint32_t*>(lds);
    float* const facc = reinterpret_cast<float*>(lds);
    uint8_t* const un = lds + L::kAcc;
    uint64_t* const cand = reinterpret_cast<uint64_t*>(un);
    uint32_t* const tmax = reinterpret_cast<uint32_t*>(un + L::kUnion);
    uint32_t* const wmax = tmax + NT;
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(un + L::kUnion + L::kTmax);
    const uint32_t tid = threadIdx.x;
    const uint32_t tile = blockIdx.x / a.nq, q = blockIdx.x % a.nq;
    const uint64_t doc0 = (uint64_t)tile * TILE_DOCS;
    const uint32_t ndocs_tile = (uint32_t)min((uint64_t)TILE_DOCS, a.n_docs - doc0);
    const int rounds = (int)((ndocs_tile + 4 * NT - 1) / (4 * NT));
    const uint64_t* sk = a.s_keys + (uint64_t)q * a.depth;
    const uint32_t* di = a.d_idx + (uint64_t)q * a.depth;
    const uint32_t* dk = a.d_key + (uint64_t)q * a.depth;
    const int32_t dn = a.d_n[q];
    const uint32_t self = a.self_ord ? (uint32_t)a.self_ord[q] : 0xFFFFFFFFu;

    for (int i = tid; i < rounds * 4 * NT; i += NT) {
        facc[i] = 0.f;
        member[i] = 0;
    }
    __shared__ uint32_t mmu[4];  // min / max sparse score, min / max dense key (the lists come in any order)
    if (tid < 64) ss.cnt[tid] = 0;
    if (tid == 0) {
        ss.n_cand = 0;
        ss.tau0 = 1;
        ss.smax = 0;
        mmu[0] = 0xFFFFFFFFu;
        mmu[1] = 0;
        mmu[2] = 0xFFFFFFFFu;
        mmu[3] = 0;
    }
    __syncthreads();
    {
        uint32_t lo_s = 0xFFFFFFFFu, hi_s = 0, lo_d = 0xFFFFFFFFu, hi_d = 0;
        for (uint32_t j = tid; j < a.depth; j += NT) {
            const uint64_t key = sk[j];
            if (key) {
                const uint32_t sc = (uint32_t)(key >> 32);
                lo_s = min(lo_s, sc);
                hi_s = max(hi_s, sc);
            }
            if ((int)j < dn) {
                lo_d = min(lo_d, dk[j]);
                hi_d = max(hi_d, dk[j]);
            }
        }
        // wave reductions (DPP) first, then one LDS atomic per wave and quantity (min x = ~max ~x)
        lo_s = ~wave_max_u32(~lo_s);
        hi_s = wave_max_u32(hi_s);
        lo_d = ~wave_max_u32(~lo_d);
        hi_d = wave_max_u32(hi_d);
        if ((tid & 63u) == 0) {
            if (hi_s) {
                atomicMin(&mmu[0], lo_s);
                atomicMax(&mmu[1], hi_s);
            }
            if (hi_d) {
                atomicMin(&mmu[2], lo_d);
                atomicMax(&mmu[3], hi_d);
            }
        }
    }
    __syncthreads();
    // The fusion arithmetic of the contract (include/msr.h, msr_hybrid_search), the one hybrid_tiles and
    // hybrid_fuse_query compute: reciprocal of the spread, EXACTLY 1 at the list's maximum (the sparse comparison on the
    // u32 score), two fused adds from +0. Every thread derives the per-side constants for itself.
    const uint32_t smax_u = mmu[1];
    const bool has_s = smax_u != 0, has_d = mmu[3] != 0;  // (sparse scores and dense keys of hits are non-zero)
    const float smax = has_s ? (float)smax_u : 0.f, smin = has_s ? (float)mmu[0] : 0.f;
    const float dmax = has_d ? key_to_f32(mmu[3]) + 0.0f : 0.f, dmin = has_d ? key_to_f32(mmu[2]) + 0.0f : 0.f;
    const float inv_sden = 1.0f / fmaxf(smax - smin, 1e-9f), inv_dden = 1.0f / fmaxf(dmax - dmin, 1e-9f);
    const bool spread_s = smax > smin, spread_d = dmax > dmin;
    // dense pass first (the reference adds the dense term first), then the sparse pass; docs are unique per list
    for (int j = tid; j < dn; j += NT) {
        const uint32_t ord = a.row2ord[di[j]];
        if (ord != self && ord >= doc0 && ord < doc0 + ndocs_tile) {
            const float d = key_to_f32(dk[j]) + 0.0f;
            facc[ord - doc0] = __builtin_fmaf(a.w_dense, (d == dmax && spread_d) ? 1.0f : (d - dmin) * inv_dden, 0.f);
            member[ord - doc0] = 1;
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < a.depth; j += NT) {
        const uint64_t key = sk[j];
        if (!key) continue;
        const uint32_t ord = 0xFFFFFFFFu - (uint32_t)key;
        if (ord != self && ord >= doc0 && ord < doc0 + ndocs_tile) {
            const uint32_t sv = (uint32_t)(key >> 32);
            facc[ord - doc0] = __builtin_fmaf(a.w_sparse, (sv == smax_u && spread_s) ? 1.0f : ((float)sv - smin) * inv_sden,
                                              facc[ord - doc0]);
            member[ord - doc0] = 1;
        }
    }
    __syncthreads();
    for (int i = tid; i < rounds * 4 * NT; i += NT) acc[i] = member[i] ? f32_to_key(facc[i]) : 0u;
    __syncthreads();
    tile_select<TILE_DOCS, NT, CAND>(reinterpret_cast<const uint4*>(lds), cand, tmax, wmax, ss, rounds, doc0, (int)a.k,
                                     a.part + ((uint64_t)tile * a.nq + q) * a.k, threadIdx.x);
}

}  // namespace msr

// ================================================================================================ fused hybrid tile
// Single-tile indexes (n_docs <= 8192: BASELINE config 5 is COCO-5K's 5 000 images): ONE workgroup per query does the
// whole of  sparse top-`depth`  +  dense top-`depth`  +  fuse()  +  top-k  (src/search.py:55-63,85-99,455-461,
// src/hybrid.py:32-53) without a list ever leaving the CU:
//   1. accumulate_tile: the query's exact integer scores against the tile, in LDS (the search path's own phase);
//   2. every thread takes its 16 accumulators and the same 16 docs' dense scores (one row of the GEMM's output, written
//      in ORDINAL order because the GEMM ran on the ordinal-permuted passage matrix) into registers;
//   3. hist_threshold twice: the composite of the depth-th best sparse score and of the depth-th best dense score —
//      list MEMBERSHIP is all fuse() needs (min = the depth-th score, max = the best, "doc in run");
//   4. fused score per doc from registers -> LDS tile of order-preserving keys -> tile_select(k) -> result arrays.
// What this replaces: tile_select at k = 1000 inside score_tiles, select_tiles over the 500 MB score matrix,
// fuse_tiles re-reading 2 x 25 010 x 1000 keys, and three list merges.
namespace msr {

struct HybridArgs {
    const uint32_t* dkeys;    // [qn][ld] f32 bit patterns of the dense scores of queries q0 .. q0+qn-1, by ORDINAL
    uint64_t ld;
    const int32_t* self_ord;  // [nq] ordinal to skip (remove_query) or -1; may be null
    uint32_t depth, k;
    float w_dense, w_sparse;
    uint32_t* out_ord;        // [nq][k]
    float* out_score;         // [nq][k] fused scores
    int32_t* out_n;           // [nq]
    // ---- multi-tile indexes (MODE 1 of hybrid_tiles + hybrid_fuse_query): per (launch row, tile) candidate lists
    const uint32_t* qlist;    // launch row -> query of the batch (second round: the flagged queries), or null: q0 + row
    // candidate RECORDS, [rows][n_tiles][stride] each: a doc that is a candidate for either depth list of its tile, with
    // its sparse score (0: not a sparse candidate) and the key of its dense score (0: not a dense candidate)
    uint32_t* rec_ord;        // doc ordinal (0xFFFFFFFF = empty slot)
    uint32_t* rec_s;
    uint32_t* rec_d;
    uint4* tile_meta;         // [rows][n_tiles][2]: {weakest emitted sparse composite (lo, hi), present sparse scores, all
                              //   emitted?}, {weakest emitted dense composite (lo, hi), docs of the tile, all emitted?}
    uint32_t n_tiles;         // tiles of the index
    uint32_t stride;          // record slots per (row, tile): 2 x quota_full (the union of two candidate sets)
    uint32_t quota_full;      // candidates a full tile emits per side
    uint32_t quota_last;      // ... and the (shorter) last tile
    uint32_t* flags;          // [nq] hybrid_fuse_query: 1 = the candidate lists did not cover a depth list (second round)
};

// The rare paths of hybrid_tiles, kept OUT OF LINE: inlined, the general selections' live ranges cost the common path
// ~100 spilled VGPRs (measured: 316 -> 20 bytes of scratch per lane). `keys` is the thread-interleaved tile of u32 keys
// (LDS accumulators, or the query's row of dense scores — f32 bit patterns — in global memory); dense scores become
// order-preserving keys, canonicalised like the fast path's floats (-0 = +0), docs past the corpus are masked out.
template <int TILE_DOCS, int NT>
__device__ __attribute__((noinline)) uint64_t threshold_general(const uint32_t* keys, int rounds, uint32_t ndocs, uint32_t k,
                                                                bool dense, uint32_t* hist, uint64_t* cand, HistScratch* hs,
                                                                uint32_t tid) {
    const HistResult g = hist_threshold<TILE_DOCS, NT>(
        [&](int r) {
            uint4 x = r < rounds ? reinterpret_cast<const uint4*>(keys)[r * NT + tid] : make_uint4(0, 0, 0, 0);
            if (dense) {
                uint32_t k4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t local = 4u * ((uint32_t)r * NT + tid) + (uint32_t)e;
                    k4[e] = (r < rounds && local < ndocs) ? f32_to_key(__uint_as_float(k4[e]) + 0.0f) : 0u;
                }
                x = make_uint4(k4[0], k4[1], k4[2], k4[3]);
            }
            return x;
        },
        k, hist, cand, *hs, tid,
        [dense](uint32_t key, uint32_t lo) { return dense ? key_to_f32(key) - key_to_f32(lo) : (float)(key - lo); });
    return g.T > 1 ? g.T : ((uint64_t)g.kmin << 13);  // (everything present belongs: the smallest key, any doc)
}

template <int TILE_DOCS, int NT, int CAND>
__device__ __attribute__((noinline)) void tile_select_general(const uint4* a4, uint64_t* cand, uint32_t* tmax, uint32_t* wmax,
                                                              SelectScratch* ss, int rounds, int k, uint64_t* out,
                                                              uint32_t tid) {
    tile_select<TILE_DOCS, NT, CAND>(a4, cand, tmax, wmax, *ss, rounds, 0ull, k, out, tid);
}

// scratch of the dual selection (separate from the tile's LDS carve, which accumulate_tile and tile_select own)
struct DualScratch {
    uint32_t red[8];      // smax, ~smin', scount, key(dmax), ~key(dmin), member count, -, -   (LDS atomics, one per wave)
    uint32_t wtot[2][8];  // per-side wave totals of the bin scan
    uint32_t bin[2], above[2], cnt[2], ncand[2];
    uint64_t T[2];        // threshold composites  key << 13 | (TILE_DOCS - 1 - local)
    uint32_t fbin, fabove, fcnt, fn;  // final top-k: bin of the k-th best fused score, members above it, in it, collected
};

// MODE 0: the fused single-tile kernel described above, grid = (queries).
// MODE 1: multi-tile indexes, grid = (launch rows, tiles) like score_tiles: steps 1-3 for ONE tile with the tile's
//   candidate QUOTA in the place of the depth, then every element at or above the two quota thresholds is written to the
//   (row, tile) candidate lists; hybrid_fuse_query (below) finishes the query. Exact by verification: the quota is the
//   tile's expected share of a depth list plus five standard deviations; a query whose depth-th best lies below some
//   tile's weakest candidate is flagged and repeated with quota = depth (every tile's own top-depth: always enough).
template <int TILE_DOCS, int NT, int U, int MIN_WAVES, int MODE = 0>
__global__ __launch_bounds__(NT, MIN_WAVES) void hybrid_tiles(const ScoreArgs a, const HybridArgs h) {
    constexpr int CAND = 1024;
    constexpr int E = TILE_DOCS / NT, R = E / 4, NW = NT / 64, HW = NW / 2;
    constexpr int BPT = kHistBins / (HW * 64);  // bins per scanning thread (half of the workgroup scans each side)
    static_assert(BPT == 4 || BPT == 8, "the scan reads its bins as one or two 16-byte vectors");
    using L = TileLds<TILE_DOCS, NT, CAND>;
    static_assert(L::kUnion >= 2 * kHistBins * 4 && L::kUnion >= 2 * kHistCand * 8, "two histograms / candidate lists");
    static_assert(L::kTmax >= (int)sizeof(HistScratch), "the fallback selection's scratch lives in the maxima region");
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::kTotal];
    __shared__ DualScratch ds;
    __shared__ uint64_t res[64];
    uint32_t* const acc = reinterpret_cast<uint32_t*>(lds);
    uint8_t* const un = lds + L::kAcc;
    uint64_t* const cand = reinterpret_cast<uint64_t*>(un);
    uint32_t* const tmax = reinterpret_cast<uint32_t*>(un + L::kUnion);
    uint32_t* const wmax = tmax + NT;
    SelectScratch& ss = *reinterpret_cast<SelectScratch*>(un + L::kUnion + L::kTmax);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(un);            // [2][kHistBins]: sparse, dense
    uint64_t* const cands = reinterpret_cast<uint64_t*>(un);           // [2][kHistCand] once the scan is over
    HistScratch& hs = *reinterpret_cast<HistScratch*>(tmax);

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63, wave = rfl(tid >> 6);
    const uint32_t q = (MODE == 1 && h.qlist) ? h.qlist[blockIdx.x] : a.q0 + blockIdx.x;
    const uint32_t tile_l = MODE == 1 ? blockIdx.y : 0u;  // (the hybrid paths take whole indexes: local tile = global tile)
    const uint64_t doc0 = (uint64_t)tile_l * TILE_DOCS;
    const uint32_t ndocs = MODE == 1 ? (uint32_t)min((uint64_t)TILE_DOCS, a.n_docs - doc0) : (uint32_t)a.n_docs;
    const int rounds = (int)((ndocs + 4 * NT - 1) / (4 * NT));
    uint4* const a4 = reinterpret_cast<uint4*>(acc);
    if (tid < 8) ds.red[tid] = 0;  // (ordered before their first use by accumulate_tile's barriers)
    if (tid < 2) ds.ncand[tid] = 0;
    if (tid == 0) ds.fn = 0;
    accumulate_tile<TILE_DOCS, NT, U>(a, q, tile_l, rounds, lds, ss, tid);

    // ---- the query's row of dense scores (the GEMM wrote the f32 values in ORDINAL order) in registers; docs past the
    // corpus become NaN: min / max skip them, every comparison with them is false
    float df[E];
    {
        const uint4* row = reinterpret_cast<const uint4*>(h.dkeys + (uint64_t)blockIdx.x * h.ld + doc0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint4 x = r < rounds ? row[r * NT + tid] : make_uint4(0, 0, 0, 0);
            const uint32_t k4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t local = 4u * ((uint32_t)r * NT + tid) + (uint32_t)e;
                // (+ 0.0f: -0 and +0 are one score; they would be two keys)
                df[4 * r + e] = (r < rounds && local < ndocs) ? __uint_as_float(k4[e]) + 0.0f : __builtin_nanf("");
            }
        }
    }
    // zero both histograms (the staging arrays of the accumulation lived here)
    for (int i = tid; i < 2 * kHistBins / 4; i += NT) reinterpret_cast<uint4*>(hist)[i] = make_uint4(0, 0, 0, 0);
    // ---- pass A: present sparse scores (count, max, min) and dense scores (max, min)
    {
        uint32_t smx = 0, smn1 = 0xFFFFFFFFu, scnt = 0;
        float dmx = -__builtin_inff(), dmn = __builtin_inff();
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < rounds) {
                const uint4 x = a4[r * NT + tid];
                const uint32_t s4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    smx = max(smx, s4[e]);
                    smn1 = min(smn1, s4[e] - 1u);  // an absent score (0) wraps to the largest value
                    scnt += min(s4[e], 1u);
                    dmx = fmaxf(dmx, df[4 * r + e]);
                    dmn = fminf(dmn, df[4 * r + e]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        smx = wave_max_u32(smx);
        smn1 = wave_max_u32(~smn1);
        scnt = wave_sum_u32(scnt);
        const uint32_t kx = wave_max_u32(f32_to_key(dmx)), kn = wave_max_u32(~f32_to_key(dmn));
        if (lane == 0) {
            atomicMax(&ds.red[0], smx);
            atomicMax(&ds.red[1], smn1);
            atomicAdd(&ds.red[2], scnt);
            atomicMax(&ds.red[3], kx);
            atomicMax(&ds.red[4], kn);
        }
    }
    __syncthreads();
    const uint32_t smax_u = ds.red[0], n_s = ds.red[2];
    const uint32_t smin_u = n_s ? ~ds.red[1] + 1u : 0u;
    const uint32_t n_d = ndocs;  // every doc has a dense score
    const float dmax_f = key_to_f32(ds.red[3]), dmin_all = key_to_f32(~ds.red[4]);
    // list sizes: the depth best (MODE 1: the tile's quota of candidates), or everything that is present
    const uint32_t want = MODE == 1 ? (tile_l + 1 == h.n_tiles ? h.quota_last : h.quota_full) : h.depth;
    const uint32_t need_s = min(want, n_s), need_d = min(want, n_d);
    // ---- pass B: histograms, linear between the smallest and the largest present value of each side (an absent
    // sparse score, 0, saturates to bin 0, a doc past the corpus, NaN, converts to bin 0: harmless, the chosen bin's
    // candidates are filtered by presence). Branch-free: one fused multiply-add,
    // one conversion and one LDS add per element and side.
    const float sc_s = ((float)kHistBins - 0.5f) / (float)(smax_u - smin_u);
    const float sc_d = ((float)kHistBins - 0.5f) / (dmax_f - dmin_all);
    const bool flat_s = smax_u == smin_u, flat_d = !(dmax_f > dmin_all);  // all equal: no spread to bin on
    const uint32_t one_s = flat_s ? 0u : 1u, one_d = flat_d ? 0u : 1u;
    auto pack_u16 = [](uint32_t lo, uint32_t hi) -> uint32_t {
        typedef unsigned short us2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, (us2)__builtin_amdgcn_cvt_pk_u16(lo, hi));  // v_cvt_pk_u16_u32 saturates
    };
    uint32_t bins[E];  // sparse bin | dense bin << 16
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r < rounds) {
            const uint4 x = a4[r * NT + tid];
            const uint32_t s4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // (x - min) * scale, not fma(x, scale, -min * scale): the rounded offset of a tight cluster far from 0
                // (sparse 2e7 +- 300, dense 138.5469 +- 3e-5) puts the top bin past the array; clamped besides
                const uint32_t bs = min((uint32_t)(((float)s4[e] - (float)smin_u) * sc_s), (uint32_t)(kHistBins - 1));  // absent (0) -> 0
                const uint32_t bd = min((uint32_t)((df[4 * r + e] - dmin_all) * sc_d), (uint32_t)(kHistBins - 1));      // NaN -> 0
                atomicAdd(&hist[flat_s ? 0u : bs], one_s);
                atomicAdd(&hist[kHistBins + (flat_d ? 0u : bd)], one_d);
                bins[4 * r + e] = pack_u16(bs, bd);
            }
            __builtin_amdgcn_sched_barrier(0);  // one round at a time: hoisting all four rounds' loads costs ~50 spills
        }
    __syncthreads();
    // ---- scan: waves [0, HW) walk the sparse bins from the top, waves [HW, NW) the dense bins; the thread whose bins
    // hold the need-th best publishes {bin, elements above it, elements in it}
    {
        const uint32_t side = wave >= (uint32_t)HW ? 1u : 0u;
        const uint32_t t2 = tid - side * (HW * 64);  // thread index inside its half
        const uint32_t need = side ? need_d : need_s;
        const uint32_t* hb_base = hist + side * kHistBins + (kHistBins - BPT) - BPT * t2;  // bins ascending in memory
        uint32_t hb[BPT];  // descending bin order
        {
            const uint4 v = *reinterpret_cast<const uint4*>(hb_base + (BPT - 4));
            hb[0] = v.w, hb[1] = v.z, hb[2] = v.y, hb[3] = v.x;
            if (BPT == 8) {
                const uint4 u = *reinterpret_cast<const uint4*>(hb_base);
                hb[BPT - 4] = u.w, hb[BPT - 3] = u.z, hb[BPT - 2] = u.y, hb[BPT - 1] = u.x;
            }
        }
        uint32_t s = 0;
#pragma unroll
        for (int i = 0; i < BPT; ++i) s += hb[i];
        const uint32_t inc = wave_inclusive_scan_u32(s);
        if (lane == 63) ds.wtot[side][wave - side * HW] = inc;
        __syncthreads();
        uint32_t above = inc - s;
#pragma unroll
        for (int w = 0; w < HW; ++w) above += (uint32_t)w < wave - side * HW ? ds.wtot[side][w] : 0u;
        if (above < need && need <= above + s) {  // exactly one thread per side (none when the side is flat / empty)
            uint32_t b = 0, ab = above;
#pragma unroll
            for (int i = 0; i < BPT - 1; ++i)
                if (b == (uint32_t)i && ab + hb[i] < need) {
                    ab += hb[i];
                    b = (uint32_t)i + 1;
                }
            uint32_t cnt = hb[0];
#pragma unroll
            for (int i = 1; i < BPT; ++i) cnt = b == (uint32_t)i ? hb[i] : cnt;
            ds.bin[side] = (uint32_t)(kHistBins - 1) - (BPT * t2 + b);
            ds.above[side] = ab;
            ds.cnt[side] = cnt;
        }
    }
    __syncthreads();
    // ---- pass C: the chosen bins' elements as composites  key << 13 | (TILE_DOCS - 1 - local)  (ties: lower ordinal)
    const uint32_t bsel_s = ds.bin[0], bsel_d = ds.bin[1], cnt_s = ds.cnt[0], cnt_d = ds.cnt[1];
    const bool fast_s = !flat_s && n_s != 0 && cnt_s <= (uint32_t)kHistCand;
    const bool fast_d = !flat_d && cnt_d <= (uint32_t)kHistCand;
    {
        // which of this thread's elements sit in a chosen bin: bit j (sparse), bit 16 + j (dense); almost always none
        const uint32_t want = pack_u16(fast_s ? bsel_s : 0xFFFEu, fast_d ? bsel_d : 0xFFFEu);
        uint32_t hit = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint32_t x = bins[j] ^ want;  // a zero half = that side's bin matches
            hit |= ((x & 0xFFFFu) == 0 ? 1u : 0u) << j;
            hit |= ((x >> 16) == 0 ? 1u : 0u) << (16 + j);
        }
        if (hit) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r < rounds) {
                    const uint4 x = a4[r * NT + tid];
                    const uint32_t s4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = 4 * r + e;
                        const uint64_t inv = (uint64_t)(TILE_DOCS - 1 - (4u * ((uint32_t)r * NT + tid) + (uint32_t)e));
                        if ((hit >> j & 1u) && s4[e] != 0)
                            cands[atomicAdd(&ds.ncand[0], 1u)] = ((uint64_t)s4[e] << 13) | inv;
                        if ((hit >> (16 + j) & 1u) && df[j] == df[j])
                            cands[kHistCand + atomicAdd(&ds.ncand[1], 1u)] = ((uint64_t)f32_to_key(df[j]) << 13) | inv;
                    }
                }
        }
    }
    __syncthreads();
    // ---- exact rank inside the chosen bin: one wave per side while the bin holds <= 64 elements
    auto rank_side = [&](uint32_t side, uint32_t cnt, uint32_t need_in_bin) {
        const uint64_t* c = cands + side * kHistCand;
        if (cnt <= 64) {
            if (wave == side * HW) {
                const uint64_t me = lane < cnt ? c[lane] : 0ull;
                const uint32_t lo = (uint32_t)me, hi = (uint32_t)(me >> 32);
                uint32_t rank = 0;
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint64_t o = ((uint64_t)rdl(hi, i) << 32) | rdl(lo, i);
                    rank += o > me;
                }
                if (lane < cnt && rank == need_in_bin - 1) ds.T[side] = me;
            }
        } else {
            for (uint32_t i = tid; i < cnt; i += NT) {
                const uint64_t me = c[i];
                uint32_t rank = 0;
                for (uint32_t o = 0; o < cnt; ++o) rank += c[o] > me;
                if (rank == need_in_bin - 1) ds.T[side] = me;
            }
        }
    };
    // (the number actually collected: bin 0's count also holds the absent elements that were binned there)
    if (fast_s) rank_side(0, ds.ncand[0], need_s - ds.above[0]);
    if (fast_d) rank_side(1, ds.ncand[1], need_d - ds.above[1]);
    __syncthreads();
    uint64_t T_s = ds.T[0], T_d = ds.T[1];
    // ---- rare: a side without spread, or a bin with more than kHistCand elements (mass ties): the general selection
    if (__builtin_expect(n_s != 0 && !fast_s, 0))  // (uniform, rare)
        T_s = threshold_general<TILE_DOCS, NT>(acc, rounds, ndocs, want, false, hist, cand + kHistBins / 2, &hs, tid);
    if (__builtin_expect(!fast_d, 0))
        T_d = threshold_general<TILE_DOCS, NT>(h.dkeys + (uint64_t)blockIdx.x * h.ld + doc0, rounds, ndocs, want, true, hist,
                                               cand + kHistBins / 2, &hs, tid);
    if constexpr (MODE == 1) {
        // ---- the tile's candidates: every element at or above its side's threshold composite (exactly need_s / need_d
        // of them: composites are unique) becomes ONE record {ordinal, sparse score or 0, dense key or 0} — a doc that
        // is a candidate on both sides arrives at hybrid_fuse_query already joined
        __syncthreads();  // (everyone has read ds.ncand / ds.T of the selection)
        if (tid < 2) ds.ncand[tid] = 0;
        __syncthreads();
        const uint64_t slot0 = ((uint64_t)blockIdx.x * h.n_tiles + tile_l) * h.stride;
        uint32_t* const ro = h.rec_ord + slot0;
        uint32_t* const rs = h.rec_s + slot0;
        uint32_t* const rd = h.rec_d + slot0;
        const uint32_t ts_key = (uint32_t)(T_s >> 13), ts_inv = (uint32_t)T_s & 8191u;
        const uint32_t td_inv = (uint32_t)T_d & 8191u;
        const float td_f = key_to_f32((uint32_t)(T_d >> 13)) + 0.0f;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < rounds) {
                const uint4 x = a4[r * NT + tid];
                const uint32_t s4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t local = 4u * ((uint32_t)r * NT + tid) + (uint32_t)e;
                    const uint32_t inv = (uint32_t)(TILE_DOCS - 1) - local;
                    const float d = df[4 * r + e];
                    const bool is_s = need_s && s4[e] != 0 && (s4[e] > ts_key || (s4[e] == ts_key && inv >= ts_inv));
                    const bool is_d = d > td_f || (d == td_f && inv >= td_inv);  // (NaN = past the corpus: never)
                    if (is_s || is_d) {
                        const uint32_t pos = atomicAdd(&ds.ncand[0], 1u);
                        if (pos < h.stride) {
                            ro[pos] = (uint32_t)(doc0 + local);
                            rs[pos] = is_s ? s4[e] : 0u;
                            rd[pos] = is_d ? f32_to_key(d) : 0u;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        __syncthreads();
        for (uint32_t i = min(ds.ncand[0], h.stride) + tid; i < h.stride; i += NT) {  // empty slots
            ro[i] = 0xFFFFFFFFu;
            rs[i] = 0u;
            rd[i] = 0u;
        }
        if (tid == 0) {
            // weakest emitted element of each side as a global composite; "all emitted" = the list holds everything the
            // tile has (no threshold to respect)
            const uint32_t tl_s = (uint32_t)(TILE_DOCS - 1) - ts_inv, tl_d = (uint32_t)(TILE_DOCS - 1) - td_inv;
            const uint64_t ws = ((uint64_t)ts_key << 32) | (0xFFFFFFFFu - (uint32_t)(doc0 + tl_s));
            const uint64_t wd = ((uint64_t)(uint32_t)(T_d >> 13) << 32) | (0xFFFFFFFFu - (uint32_t)(doc0 + tl_d));
            uint4* m = h.tile_meta + ((uint64_t)blockIdx.x * h.n_tiles + tile_l) * 2;
            m[0] = make_uint4((uint32_t)ws, (uint32_t)(ws >> 32), n_s, need_s == n_s ? 1u : 0u);
            m[1] = make_uint4((uint32_t)wd, (uint32_t)(wd >> 32), n_d, need_d == n_d ? 1u : 0u);
        }
        return;
    }
    // ---- fusion (src/hybrid.py:32-53): min = the last member's score, max = the best, per side; fused keys go to the
    // accumulator tile (each thread rewrites only what it has read) and into a histogram over [fmin, fmax]
    const uint32_t ts_key = (uint32_t)(T_s >> 13), ts_inv = (uint32_t)T_s & 8191u;
    const uint32_t td_inv = (uint32_t)T_d & 8191u;
    const float td_f = key_to_f32((uint32_t)(T_d >> 13)) + 0.0f;
    const float smin = n_s ? (float)ts_key : 0.f, smax = n_s ? (float)smax_u : 0.f;
    const float dmin = td_f, dmax = dmax_f;
    const float sden = fmaxf(smax - smin, 1e-9f), dden = fmaxf(dmax - dmin, 1e-9f);
    const uint32_t self = h.self_ord ? (uint32_t)h.self_ord[q] : 0xFFFFFFFFu;
    // fused scores lie in [min(w,0) sums, max(w,0) sums]
    const float f_lo = fminf(h.w_dense, 0.f) + fminf(h.w_sparse, 0.f), f_hi = fmaxf(h.w_dense, 0.f) + fmaxf(h.w_sparse, 0.f);
    const float sc_f = ((float)kHistBins - 0.5f) / fmaxf(f_hi - f_lo, 1e-30f), of_f = -f_lo * sc_f;
    // w * ((x - min) / den) with the division as a multiplication by 1 / den (<= 1 ulp from the quotient, far inside the
    // 1e-5 the fused scores are held to) — but EXACTLY 1 at x = max, as the quotient is: with alpha = 0.5 the best
    // dense-only doc and the best sparse-only doc tie at exactly 0.5 in the reference, and that tie must stay a tie
    // (it is then broken like every other: lower ordinal first)
    const float inv_dden = 1.0f / dden, inv_sden = 1.0f / sden;
    const bool spread_d = dmax > dmin, spread_s = smax > smin;  // (max == min: every quotient is 0 / 1e-9 = 0)
    for (int i = tid; i < kHistBins / 4; i += NT) reinterpret_cast<uint4*>(hist)[i] = make_uint4(0, 0, 0, 0);
    if (tid < 64) ss.cnt[tid] = 0;
    if (tid == 0) {
        ss.n_cand = 0;
        ss.tau0 = 1;
        ss.smax = 0;
    }
    __syncthreads();  // histogram zeroed (the candidate lists that lived there are dead)
    uint32_t n_mem = 0;  // this thread's docs in the union of the two lists (without the query's own doc)
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r < rounds) {
            const uint4 x = a4[r * NT + tid];
            const uint32_t s4[4] = {x.x, x.y, x.z, x.w};
            uint32_t fk[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t local = 4u * ((uint32_t)r * NT + tid) + (uint32_t)e;
                const uint32_t inv = (uint32_t)(TILE_DOCS - 1) - local;
                const float d = df[4 * r + e];
                const bool in_d = d > td_f || (d == td_f && inv >= td_inv);
                const bool in_s = s4[e] != 0 && (s4[e] > ts_key || (s4[e] == ts_key && inv >= ts_inv));
                float f = 0.f;  // the reference adds the dense term first (runs = [dense, sparse], src/search.py:459)
                // (the two adds are FUSED by contract, include/msr.h: spelled out, not left to -ffp-contract)
                if (in_d) f = __builtin_fmaf(h.w_dense, (d == dmax && spread_d) ? 1.0f : (d - dmin) * inv_dden, f);
                if (in_s)
                    f = __builtin_fmaf(h.w_sparse, (s4[e] == smax_u && spread_s) ? 1.0f : ((float)s4[e] - smin) * inv_sden, f);
                const bool member = (in_d || in_s) && local != self;
                fk[e] = member ? f32_to_key(f) : 0u;
                if (member) {
                    atomicAdd(&hist[(uint32_t)__builtin_fmaf(f, sc_f, of_f)], 1u);
                    ++n_mem;
                }
            }
            a4[r * NT + tid] = make_uint4(fk[0], fk[1], fk[2], fk[3]);
            __builtin_amdgcn_sched_barrier(0);
        }
    n_mem = wave_sum_u32(n_mem);
    if (lane == 0) atomicAdd(&ds.red[5], n_mem);
    __syncthreads();
    // ---- top-k of the fused scores: the bin of the k-th best, then every member at or above that bin is ranked
    const uint32_t n_members = ds.red[5];
    const uint32_t need_f = min(h.k, n_members);
    {
        const bool scans = wave < (uint32_t)HW;  // the first half of the workgroup walks the bins
        const uint32_t t2 = scans ? tid : 0u;
        const uint32_t* hb_base = hist + (kHistBins - BPT) - BPT * t2;
        uint32_t hb[BPT];
        {
            const uint4 v = *reinterpret_cast<const uint4*>(hb_base + (BPT - 4));
            hb[0] = v.w, hb[1] = v.z, hb[2] = v.y, hb[3] = v.x;
            if (BPT == 8) {
                const uint4 u = *reinterpret_cast<const uint4*>(hb_base);
                hb[BPT - 4] = u.w, hb[BPT - 3] = u.z, hb[BPT - 2] = u.y, hb[BPT - 1] = u.x;
            }
        }
        uint32_t s = 0;
#pragma unroll
        for (int i = 0; i < BPT; ++i) s += hb[i];
        const uint32_t inc = wave_inclusive_scan_u32(s);
        if (scans && lane == 63) ds.wtot[0][wave] = inc;
        __syncthreads();
        uint32_t above = inc - s;
#pragma unroll
        for (int w = 0; w < HW; ++w) above += (uint32_t)w < wave ? ds.wtot[0][w] : 0u;
        if (scans && need_f != 0 && above < need_f && need_f <= above + s) {
            uint32_t b = 0, ab = above;
#pragma unroll
            for (int i = 0; i < BPT - 1; ++i)
                if (b == (uint32_t)i && ab + hb[i] < need_f) {
                    ab += hb[i];
                    b = (uint32_t)i + 1;
                }
            uint32_t cnt = hb[0];
#pragma unroll
            for (int i = 1; i < BPT; ++i) cnt = b == (uint32_t)i ? hb[i] : cnt;
            const uint32_t fb = (uint32_t)(kHistBins - 1) - (BPT * tid + b);
            ds.fbin = fb;
            ds.fabove = ab;
            ds.fcnt = cnt + (fb ? hist[fb - 1] : 0u);  // ... and the bin below it: the collection's margin (see there)
        }
    }
    __syncthreads();
    // Members at or above the k-th best's bin, plus the bin below: the fused keys are re-read from the tile (nothing is
    // kept in registers across the scan) and compared with the KEY of the lower edge of bin fbin - 1 — one whole bin of
    // margin against the rounding of the bin function, so that every member of bins >= fbin is collected.
    const uint32_t n_top_est = need_f ? ds.fabove + ds.fcnt : 0u;
    uint64_t* const top = reinterpret_cast<uint64_t*>(tmax);  // 64 keys
    bool ranked = false;
    if (__builtin_expect(n_top_est <= 60, 1)) {
        const uint32_t fbin = ds.fbin;
        const uint32_t key_edge = fbin > 1 ? f32_to_key(((float)fbin - 1.0f) / sc_f + f_lo) : 1u;
        if (need_f) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r < rounds) {
                    const uint4 x = a4[r * NT + tid];
                    const uint32_t k4[4] = {x.x, x.y, x.z, x.w};
                    if (max(max(k4[0], k4[1]), max(k4[2], k4[3])) >= key_edge) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (k4[e] != 0 && k4[e] >= key_edge) {
                                const uint32_t local = 4u * ((uint32_t)r * NT + tid) + (uint32_t)e;
                                const uint32_t pos = atomicAdd(&ds.fn, 1u);
                                if (pos < 64) top[pos] = ((uint64_t)k4[e] << 32) | (uint64_t)(0xFFFFFFFFu - local);
                            }
                    }
                }
        }
        __syncthreads();
        ranked = ds.fn <= 64;  // (a key on the very edge can add one or two to the estimate; more than 64: general path)
    }
    if (__builtin_expect(ranked, 1)) {
        const uint32_t n_top = ds.fn;
        if (tid < 64) {
            const uint64_t me = tid < n_top ? top[tid] : 0ull;
            const uint32_t lo = (uint32_t)me, hi = (uint32_t)(me >> 32);
            uint32_t rank = 0;
            for (uint32_t i = 0; i < n_top; ++i) {
                const uint64_t o = ((uint64_t)rdl(hi, i) << 32) | rdl(lo, i);
                rank += o > me;
            }
            const uint64_t o = (uint64_t)q * h.k;
            if (tid < n_top && rank < h.k) {
                h.out_ord[o + rank] = 0xFFFFFFFFu - (uint32_t)me;
                h.out_score[o + rank] = key_to_f32((uint32_t)(me >> 32));
            }
            if (tid >= need_f && tid < h.k) {
                h.out_ord[o + tid] = 0xFFFFFFFFu;
                h.out_score[o + tid] = 0.f;
            }
            if (tid == 0) h.out_n[q] = (int32_t)need_f;
        }
        return;
    }
    // ---- rare (many equal fused scores around the k-th place): the general tile selection over the fused keys
    tile_select_general<TILE_DOCS, NT, CAND>(a4, cand, tmax, wmax, &ss, rounds, (int)h.k, res, tid);
    __syncthreads();
    if (tid < h.k) {
        const uint64_t key = res[tid];
        const uint64_t o = (uint64_t)q * h.k + tid;
        h.out_ord[o] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
        h.out_score[o] = key ? key_to_f32((uint32_t)(key >> 32)) : 0.f;
    }
    if (tid < 64) {
        const uint32_t nh = (uint32_t)__popcll(__ballot(tid < h.k && res[tid] != 0));
        if (tid == 0) h.out_n[q] = (int32_t)nh;
    }
}

// ------------------------------------------------------------------------------------------------ multi-tile: per query
// need-th largest of the workgroup's non-zero u64 keys (unique; 0 = empty slot; each(f) calls f(key) for every key of the
// calling thread — registers, LDS or global memory, the caller's choice), by radix passes of 8 bits over the bits
// BELOW the keys' common prefix (scores of one list differ in their low 20 bits or so: the pass that matters comes first;
// a pass ends the search as soon as the chosen bin holds <= 64 keys, which are then ranked by one wave). Returns T with
// "key belongs to the need best  <=>  key != 0 and key >= T";  *present = non-zero keys, *kmax = the largest.
// need == 0: T = ~0 (nothing belongs); need >= present: T = the smallest key (everything belongs).
struct KthScratch {
    uint32_t hist[256];
    uint64_t wmin[16], wmax[16];
    uint32_t wcnt[16];
    uint64_t small[64];
    uint32_t n_small, pad;
    uint64_t T;
};

template <int NT, class Each>
__device__ __forceinline__ uint64_t kth_largest_u64(Each each, uint32_t need, KthScratch& ks, const uint32_t tid,
                                                    uint32_t* present, uint64_t* kmax) {
    constexpr int NW = NT / 64;
    const uint32_t lane = tid & 63, wave = rfl(tid >> 6);
    uint64_t mn = ~0ull, mx = 0;
    uint32_t c = 0;
    each([&](const uint64_t key) {
        if (key) {
            mn = key < mn ? key : mn;
            mx = key > mx ? key : mx;
            ++c;
        }
    });
    mn = ~wave_max_u64(~mn);
    mx = wave_max_u64(mx);
    c = wave_sum_u32(c);
    __syncthreads();  // previous users of the scratch are done
    if (lane == 0) {
        ks.wmin[wave] = mn;
        ks.wmax[wave] = mx;
        ks.wcnt[wave] = c;
    }
    if (tid == 0) ks.n_small = 0;
    __syncthreads();
    mn = ~0ull, mx = 0, c = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        mn = ks.wmin[w] < mn ? ks.wmin[w] : mn;
        mx = ks.wmax[w] > mx ? ks.wmax[w] : mx;
        c += ks.wcnt[w];
    }
    *present = c;
    *kmax = mx;
    if (need == 0 || c == 0) return ~0ull;
    if (need >= c) return mn;
    // (two or more keys, all different: mx != mn)
    const int top = 63 - __clzll((long long)(mx ^ mn));
    int shift = max(top - 7, 0);
    uint64_t hi_mask = shift + 8 >= 64 ? 0ull : ~0ull << (shift + 8);
    uint64_t prefix = mx & hi_mask;
#pragma unroll 1
    for (;;) {
        ks.hist[tid & 255u] = 0;  // (NT >= 256)
        __syncthreads();
        each([&](const uint64_t key) {
            if (key && (key & hi_mask) == prefix) atomicAdd(&ks.hist[(uint32_t)(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        // every wave finds the bin of the need-th largest for itself: lane l owns bins 4l .. 4l+3
        const uint4 hb = reinterpret_cast<const uint4*>(ks.hist)[lane];
        const uint32_t sum4 = hb.x + hb.y + hb.z + hb.w;
        const uint32_t inc = wave_inclusive_scan_u32(sum4);
        const uint32_t suf = rdl(inc, 63) - (inc - sum4);  // keys in bins >= 4 * lane: non-increasing in lane
        const uint32_t L = 63u - (uint32_t)__clzll((long long)__ballot(suf >= need));
        uint32_t above = rdl(suf, L) - rdl(sum4, L);
        const uint32_t b3 = rdl(hb.w, L), b2 = rdl(hb.z, L), b1 = rdl(hb.y, L), b0 = rdl(hb.x, L);
        uint32_t bin = 4 * L + 3, cnt = b3;
        if (above + b3 < need) {
            above += b3, bin = 4 * L + 2, cnt = b2;
            if (above + b2 < need) {
                above += b2, bin = 4 * L + 1, cnt = b1;
                if (above + b1 < need) above += b1, bin = 4 * L, cnt = b0;
            }
        }
        need -= above;  // rank inside the chosen bin, 1-based from the top
        prefix |= (uint64_t)bin << shift;
        hi_mask |= 255ull << shift;
        if (cnt <= 64 || shift == 0) {
            each([&](const uint64_t key) {
                if (key && (key & hi_mask) == prefix) ks.small[atomicAdd(&ks.n_small, 1u)] = key;
            });
            __syncthreads();
            if (tid < 64) {
                const uint64_t me = lane < cnt ? ks.small[lane] : 0ull;
                const uint32_t lo = (uint32_t)me, hi = (uint32_t)(me >> 32);
                uint32_t rank = 0;
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint64_t o = ((uint64_t)rdl(hi, i) << 32) | rdl(lo, i);
                    rank += o > me;
                }
                if (lane < cnt && rank == need - 1) ks.T = me;
            }
            __syncthreads();
            return ks.T;
        }
        shift = max(shift - 8, 0);  // (the last window may overlap bits that are already fixed: harmless)
        __syncthreads();            // everyone has read the histogram
    }
}

// Multi-tile indexes, second kernel: ONE workgroup per query finishes what hybrid_tiles<MODE 1> prepared. The query's
// candidate records (a few thousand: 4 tiles x 836 at the reference's own shape) live in REGISTERS from the first load to
// the last pass: the depth-th best of each side among them (exact when every tile's weakest candidate lies at or below
// it: checked, else the query is flagged for the second round), the reference's fusion over the union of the two lists
// (src/hybrid.py:32-53: min = the depth-th score, max = the best, of the UNFILTERED lists, src/search.py:76-81; the
// query's own doc skipped, src/search.py:72-74) — a record carries both of its doc's scores, so there is nothing to
// join — and the top-k of the fused scores (ties: lower ordinal). k <= 1024, depth <= 1024.
//
// UNION = true (msr_hybrid_search_union; `u` is read by these instances only, the others are launched with an unused
// one): the same kernel up to the fused keys, then NO top-k selection: every non-zero fused key (<= 2 x depth <= 2 048)
// is collected and sorted, h.k = 2 x depth is the row length of the outputs, and the records stay in the registers beside
// their fused keys, because the optional per-member outputs need them again after the sort: a sorted key carries the
// ordinal, not the record slot, so each thread walks its records once more and finds every member's rank by a binary
// search of its (unique) fused key in the sorted LDS array (<= 11 probes per member, ~2 000 members over 256 or 512
// threads) — no slot array to carry through the sort, no second sort.

// The optional outputs of the union pass on the device (null = not wanted): the four of msr_hybrid_search_union, and the
// exact sparse extremes that only msr_hybrid_sweep asks for
struct UnionOut {
    uint8_t* src;      // [nq][2 x depth] bit 0: in the dense depth list, bit 1: in the sparse depth list
    uint32_t* sparse;  // [nq][2 x depth] exact sparse score where bit 1 is set, else 0
    float* dense;      // [nq][2 x depth] dense score where bit 0 is set, else 0
    float* range;      // [nq][4] {dense max, dense min, sparse max, sparse min} of the unfiltered depth lists
    uint32_t* ext;     // [nq][2] {sparse max, sparse min} as exact u32 (the f32 images above can hide the maximum)
};

template <int NT, int EPT /* records per thread held in registers */, bool UNION = false>
__global__ __launch_bounds__(NT) void hybrid_fuse_query(const HybridArgs h, const uint32_t q0, const UnionOut u) {
    static_assert(NT >= 256 && NT % 64 == 0 && NT / 64 <= 16, "scratch layout");
    constexpr int CAP = UNION ? 2 * kCandCap : kCandCap;  // (a power of two: rank_and_emit's bitonic sort pads to one)
    __shared__ __attribute__((aligned(16))) uint64_t cand[CAP];
    __shared__ __attribute__((aligned(16))) uint64_t res[CAP];
    __shared__ __attribute__((aligned(16))) KthScratch ks;
    __shared__ uint32_t red[4];             // present sparse scores, docs, invalid flag, collected keys
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t row = blockIdx.x;
    const uint32_t q = h.qlist ? h.qlist[row] : q0 + row;
    const uint32_t n_slots = h.n_tiles * h.stride;
    const uint32_t* const g_ord = h.rec_ord + (uint64_t)row * n_slots;
    const uint32_t* const g_s = h.rec_s + (uint64_t)row * n_slots;
    const uint32_t* const g_d = h.rec_d + (uint64_t)row * n_slots;
    const uint4* const meta = h.tile_meta + (uint64_t)row * h.n_tiles * 2;
    // Read in a loop from global memory, every pass below would pay a dependent L2 round trip per element (measured with
    // the first version of this kernel: 0.47 ms instead of 0.3 for 5 000 queries); queries with more records than the
    // registers hold (second round on many tiles) take that loop.
    const bool in_regs = n_slots <= (uint32_t)(EPT * NT);  // (uniform)
    uint32_t ro[EPT], rs[EPT], rd[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const uint32_t i = tid + (uint32_t)e * NT;
        const bool live = in_regs && i < n_slots;
        ro[e] = live ? g_ord[i] : 0xFFFFFFFFu;
        rs[e] = live ? g_s[i] : 0u;
        rd[e] = live ? g_d[i] : 0u;
    }
    if (tid < 4) red[tid] = 0;
    __syncthreads();
    {
        uint32_t ns = 0, nd = 0;
        for (uint32_t t = tid; t < h.n_tiles; t += NT) {
            ns += meta[2 * t].z;
            nd += meta[2 * t + 1].z;
        }
        ns = wave_sum_u32(ns);
        nd = wave_sum_u32(nd);
        if (lane == 0 && (ns | nd)) {
            atomicAdd(&red[0], ns);
            atomicAdd(&red[1], nd);
        }
    }
    __syncthreads();
    const uint32_t need_s = min(h.depth, red[0]), need_d = min(h.depth, red[1]);
    // visit(f): f(ordinal, sparse score, dense key) for every record of this thread
    auto visit = [&](auto f) {
        if (in_regs) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) f(ro[e], rs[e], rd[e]);
        } else {
            for (uint32_t i = tid; i < n_slots; i += NT) f(g_ord[i], g_s[i], g_d[i]);
        }
    };
    auto comp = [](uint32_t v, uint32_t ord) -> uint64_t { return v ? ((uint64_t)v << 32) | (uint64_t)(0xFFFFFFFFu - ord) : 0ull; };
    auto each_s = [&](auto f) { visit([&](uint32_t o, uint32_t sv, uint32_t) { f(comp(sv, o)); }); };
    auto each_d = [&](auto f) { visit([&](uint32_t o, uint32_t, uint32_t dv) { f(comp(dv, o)); }); };
    uint32_t c_s, c_d;
    uint64_t mx_s, mx_d;
    const uint64_t T_s = kth_largest_u64<NT>(each_s, need_s, ks, tid, &c_s, &mx_s);
    const uint64_t T_d = kth_largest_u64<NT>(each_d, need_d, ks, tid, &c_d, &mx_d);
    // ---- are the lists complete? a tile that did not emit everything it has must have its weakest candidate at or
    // below the side's depth-th best
    {
        bool bad = c_s < need_s || c_d < need_d;
        for (uint32_t t = tid; t < h.n_tiles; t += NT) {
            const uint4 a = meta[2 * t], b = meta[2 * t + 1];
            if (need_s && !a.w && T_s < (((uint64_t)a.y << 32) | a.x)) bad = true;
            if (need_d && !b.w && T_d < (((uint64_t)b.y << 32) | b.x)) bad = true;
        }
        if (bad) red[2] = 1;  // (benign race: every writer stores 1)
    }
    __syncthreads();
    if (red[2]) {  // (uniform) second round: hybrid_tiles<MODE 1> with quota = depth for this query
        if (tid == 0) {
            h.flags[q] = 1;
            h.out_n[q] = 0;
        }
        return;
    }
    // ---- fusion (src/hybrid.py:32-53; the dense term first: runs = [dense, sparse], src/search.py:459)
    const uint32_t self = h.self_ord ? (uint32_t)h.self_ord[q] : 0xFFFFFFFFu;
    const uint32_t smax_u = (uint32_t)(mx_s >> 32), smin_u = need_s ? (uint32_t)(T_s >> 32) : 0u;
    const float smax = need_s ? (float)smax_u : 0.f, smin = (float)smin_u;
    const float dmax = need_d ? key_to_f32((uint32_t)(mx_d >> 32)) + 0.0f : 0.f;
    const float dmin = need_d ? key_to_f32((uint32_t)(T_d >> 32)) + 0.0f : 0.f;
    const float inv_sden = 1.0f / fmaxf(smax - smin, 1e-9f), inv_dden = 1.0f / fmaxf(dmax - dmin, 1e-9f);
    const bool spread_s = smax > smin, spread_d = dmax > dmin;
    auto fused_key = [&](uint32_t o, uint32_t sv, uint32_t dv) -> uint64_t {
        const bool in_s = need_s && sv && comp(sv, o) >= T_s;
        const bool in_d = need_d && dv && comp(dv, o) >= T_d;
        if (!(in_s || in_d) || o == self) return 0ull;
        float f = 0.f;
        if (in_d) {  // (EXACTLY 1 at the maximum, as the reference's quotient is: see hybrid_tiles)
            const float d = key_to_f32(dv) + 0.0f;
            f = __builtin_fmaf(h.w_dense, (d == dmax && spread_d) ? 1.0f : (d - dmin) * inv_dden, f);
        }
        // (the two adds are FUSED by contract, include/msr.h: spelled out, not left to -ffp-contract)
        if (in_s) f = __builtin_fmaf(h.w_sparse, (sv == smax_u && spread_s) ? 1.0f : ((float)sv - smin) * inv_sden, f);
        return ((uint64_t)f32_to_key(f) << 32) | (uint64_t)(0xFFFFFFFFu - o);
    };
    // the fused keys replace the records in the registers (16 x u64 for 48 x u32; UNION keeps both)
    uint64_t fk[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) fk[e] = in_regs ? fused_key(ro[e], rs[e], rd[e]) : 0ull;
    auto each_f = [&](auto f) {
        if (in_regs) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) f(fk[e]);
        } else {
            for (uint32_t i = tid; i < n_slots; i += NT) f(fused_key(g_ord[i], g_s[i], g_d[i]));
        }
    };
    uint32_t n_out;
    if constexpr (UNION) {
        // ---- the whole union: every member's key, sorted (ties: lower ordinal)
        each_f([&](const uint64_t key) {
            if (key) {
                const uint32_t pos = atomicAdd(&red[3], 1u);
                if (pos < (uint32_t)CAP) cand[pos] = key;
            }
        });
        __syncthreads();
        n_out = min(min(red[3], (uint32_t)CAP), h.k);  // (each depth list holds <= depth keys: red[3] <= 2 x depth = h.k)
    } else {
        // ---- top-k of the fused scores over the union (ties: lower ordinal)
        uint32_t members;
        uint64_t mx_f;
        const uint64_t T_f = kth_largest_u64<NT>(each_f, h.k, ks, tid, &members, &mx_f);
        n_out = min(h.k, members);
        each_f([&](const uint64_t key) {
            if (key && key >= T_f) {
                const uint32_t pos = atomicAdd(&red[3], 1u);
                if (pos < (uint32_t)kCandCap) cand[pos] = key;
            }
        });
        __syncthreads();
    }
    rank_and_emit<NT, true>(cand, (int)n_out, (int)h.k, res, tid);
    __syncthreads();
    for (uint32_t i = tid; i < h.k; i += NT) {
        const uint64_t key = res[i];
        const uint64_t o = (uint64_t)q * h.k + i;
        h.out_ord[o] = key ? 0xFFFFFFFFu - (uint32_t)key : 0xFFFFFFFFu;
        h.out_score[o] = key ? key_to_f32((uint32_t)(key >> 32)) : 0.f;
    }
    if (tid == 0) {
        h.out_n[q] = (int32_t)n_out;
        h.flags[q] = 0;
    }
    if constexpr (UNION) {
        const uint64_t o = (uint64_t)q * h.k;
        if (u.range && tid == 0) {
            float* const r = u.range + (uint64_t)q * 4;
            r[0] = dmax, r[1] = dmin, r[2] = smax, r[3] = smin;
        }
        if (u.ext && tid == 0) {
            u.ext[(uint64_t)q * 2] = need_s ? smax_u : 0u;
            u.ext[(uint64_t)q * 2 + 1] = smin_u;
        }
        if (!(u.src || u.sparse || u.dense)) return;  // (uniform)
        for (uint32_t i = n_out + tid; i < h.k; i += NT) {
            if (u.src) u.src[o + i] = 0;
            if (u.sparse) u.sparse[o + i] = 0u;
            if (u.dense) u.dense[o + i] = 0.f;
        }
        // every member back to its record: the rank of its fused key in the sorted (descending, unique) keys
        auto place = [&](const uint64_t key, uint32_t ord, uint32_t sv, uint32_t dv) {
            if (!key) return;
            uint32_t lo = 0, hi = n_out;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (res[mid] > key) lo = mid + 1;
                else hi = mid;
            }
            if (lo >= n_out) return;  // (cannot happen: every non-zero key was collected)
            const bool in_s = need_s && sv && comp(sv, ord) >= T_s;
            const bool in_d = need_d && dv && comp(dv, ord) >= T_d;
            if (u.src) u.src[o + lo] = (uint8_t)((in_d ? 1u : 0u) | (in_s ? 2u : 0u));
            if (u.sparse) u.sparse[o + lo] = in_s ? sv : 0u;
            if (u.dense) u.dense[o + lo] = in_d ? key_to_f32(dv) : 0.f;
        };
        if (in_regs) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) place(fk[e], ro[e], rs[e], rd[e]);
        } else {
            for (uint32_t i = tid; i < n_slots; i += NT) {
                const uint32_t ord = g_ord[i], sv = g_s[i], dv = g_d[i];
                place(fused_key(ord, sv, dv), ord, sv, dv);
            }
        }
    }
}

// rows of the passage matrix in ORDINAL order: P_ord[row2ord[r]] = P[r]
__global__ __launch_bounds__(256) void permute_rows(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                    const uint32_t* __restrict__ row2ord, uint32_t vecs_per_row) {
    const uint32_t r = blockIdx.x;
    const uint4* s = src + (uint64_t)r * vecs_per_row;
    uint4* d = dst + (uint64_t)row2ord[r] * vecs_per_row;
    for (uint32_t i = threadIdx.x; i < vecs_per_row; i += 256) d[i] = s[i];
}

}  // namespace msr

// Bytes per row of a dense handle's passage rows and of its device query copy: h fp16 values, or hp f32 values (K zero
// padded to a multiple of kF32KStep)
static size_t dense_row_bytes(const msr_dense* dx) { return dx->f32 ? (size_t)dx->hp * 4 : (size_t)dx->h * 2; }

// Passage rows in doc-ORDINAL order (P_ord[row2ord[r]] = P[r]), so that a query's row of GEMM output lines up with the
// sparse accumulator tiles; in the handle's precision, built on first use, cached on the dense handle while the mapping
// is unchanged.
static int ensure_ordinal_rows(msr_dense* dx, hipStream_t stream, const uint32_t* row2ord, const uint64_t n) {
    if (!dx->d_P_ord || dx->ord_map.size() != n || memcmp(dx->ord_map.data(), row2ord, (size_t)n * 4) != 0) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (uint64_t r = 0; r < n; ++r) {
            if (row2ord[r] >= n || seen[row2ord[r]]) {
                set_error("row2ord is not a permutation of the doc ordinals (row %llu -> %u)", (unsigned long long)r, row2ord[r]);
                return MSR_E_INVAL;
            }
            seen[row2ord[r]] = 1;
        }
        uint32_t* d_map = nullptr;
        const size_t row_bytes = dense_row_bytes(dx), bytes = (size_t)dx->n_pad * row_bytes;  // (row_bytes % 16 == 0)
        if (!dx->d_P_ord && hipMalloc(&dx->d_P_ord, bytes) != hipSuccess) {
            dx->d_P_ord = nullptr;
            set_error("hipMalloc of %zu bytes for the ordinal-ordered passage matrix failed", bytes);
            return MSR_E_NOMEM;
        }
        bool ok = hipMalloc(&d_map, std::max<size_t>((size_t)n, 1) * 4) == hipSuccess &&
                  hipMemsetAsync(dx->d_P_ord, 0, bytes, stream) == hipSuccess &&
                  hipMemcpyAsync(d_map, row2ord, (size_t)n * 4, hipMemcpyHostToDevice, stream) == hipSuccess;
        if (ok && n) {
            const void* src = dx->f32 ? (const void*)dx->d_P32 : (const void*)dx->d_P;
            hipLaunchKernelGGL(permute_rows, dim3((uint32_t)n), dim3(256), 0, stream, reinterpret_cast<const uint4*>(src),
                               reinterpret_cast<uint4*>(dx->d_P_ord), d_map, (uint32_t)(row_bytes / 16));
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && hipStreamSynchronize(stream) == hipSuccess;
        if (d_map) (void)hipFree(d_map);
        if (!ok) {
            dx->ord_map.clear();
            set_error("building the ordinal-ordered passage matrix failed: %s", hipGetErrorString(hipGetLastError()));
            return MSR_E_HIP;
        }
        dx->ord_map.assign(row2ord, row2ord + n);
    }
    return MSR_OK;
}

// Score rows per chunk of queries of the two device-resident hybrid paths: the kernel after the GEMM reads its rows
// back out of the Infinity Cache (80 to 1 024 MB measured within noise of each other)
constexpr uint64_t kHybridChunkBytes = 160ull << 20;

// What the fused and the multi-tile path share before their launches
struct HybridSetup {
    msr_batch* b = nullptr;
    uint8_t* d_Q = nullptr;   // [nq rounded up to 256] query rows of dense_row_bytes each, zero padded
    uint32_t* d_S = nullptr;  // score rows of one chunk
    bool ok = false;          // every scratch slot was taken and every upload enqueued
    ScoreArgs sa;             // every query of the batch; the hybrid kernels write their lists through ha
    HybridArgs ha;            // the fields that both paths use
};

// Rows [0, rows) of a host query matrix ([rows][h], fp16 or f32 as the handle holds) into a device copy of rows_pad rows
// of dense_row_bytes: the padding rows, and on an f32 handle whose h is not a multiple of kF32KStep the padding columns,
// zeroed (exactly neutral in either GEMM)
static bool upload_query_rows(const msr_dense* dx, uint8_t* d_Q, const void* q, size_t rows, size_t rows_pad,
                              hipStream_t st) {
    const size_t q_row = dense_row_bytes(dx), h_row = (size_t)dx->h * (dx->f32 ? 4 : 2);
    if (q_row == h_row)
        return hipMemsetAsync(d_Q + rows * q_row, 0, (rows_pad - rows) * q_row, st) == hipSuccess &&
               hipMemcpyAsync(d_Q, q, rows * h_row, hipMemcpyHostToDevice, st) == hipSuccess;
    return hipMemsetAsync(d_Q, 0, rows_pad * q_row, st) == hipSuccess &&
           hipMemcpy2DAsync(d_Q, q_row, q, h_row, h_row, rows, hipMemcpyHostToDevice, st) == hipSuccess;
}

// The hybrid paths' GEMM: f32 bit patterns of C = Q * P_ord^T (the ordinal-ordered rows) into out[q][ld] for doc
// columns [0, n_cover), on the f32 MFMA for an f32 handle (the fmaf chain, 128 x 128 blocks), on the fp16 one otherwise
// (256 x 256 blocks where H allows); Q rows padded to qn_pad, a multiple of hybrid_gemm_block(dx). raw = false
// (msr_hybrid_deep): the same instances write the order-preserving keys of msr_dense_search instead.
static int launch_hybrid_gemm(msr_dense* dx, const uint8_t* d_Q, uint32_t* d_S, uint32_t qn, uint32_t qn_pad,
                              uint64_t n_cover, uint64_t ld, hipStream_t st, bool raw = true) {
    if (dx->f32)
        return launch_dense_gemm_f32(dx, (const float*)dx->d_P_ord, (const float*)d_Q, d_S, qn, qn_pad, n_cover, ld, st,
                                     raw);
    return launch_dense_gemm(dx, (const _Float16*)dx->d_P_ord, (const _Float16*)d_Q, d_S, qn, qn_pad, n_cover, ld, st,
                             true, raw);
}

// Query rows per GEMM block edge, the unit in which both device-resident paths size their chunks
static uint32_t hybrid_gemm_block(const msr_dense* dx) { return dx->f32 ? 128u : 256u; }

// The ordinal-ordered passage rows, the query batch (created for `batch_k`), the query matrix, `s_bytes` of score rows
// and the result lists out of the handle's scratch, the uploads of the queries (q: [nq][h], fp16 or f32 as the handle
// holds) and of self_ord, and both argument blocks. A non-zero return is an error before the batch exists; s.ok == false
// is a failed slot or upload (the caller reports it and still owns s.b).
static int hybrid_setup(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                        const void* q, int nq, int batch_k, int depth, int k, float alpha, uint32_t flags,
                        const uint32_t* row2ord, const int32_t* self_ord, uint64_t ld, size_t s_bytes, HybridSetup& s) {
    DeviceIndex* d = ix->dev;
    if (int rc = ensure_ordinal_rows(dx, d->stream, row2ord, ix->host.h->n_docs)) return rc;
    if (int rc = msr_batch_create(ix, q_ptr, q_term, q_w, nq, batch_k, flags, &s.b)) return rc;
    const uint32_t nq_pad = (uint32_t)((nq + 255) / 256 * 256);
    const size_t perk = std::max<size_t>((size_t)nq * k, 1);
    s.d_Q = (uint8_t*)dx->take(msr_dense::S_Q, std::max<size_t>((size_t)nq_pad * dense_row_bytes(dx), 16));
    s.d_S = (uint32_t*)dx->take(msr_dense::S_S, s_bytes);
    uint32_t* d_ord = (uint32_t*)dx->take(msr_dense::S_ORD, perk * 4);
    float* d_sf = (float*)dx->take(msr_dense::S_SF, perk * 4);
    int32_t* d_n = (int32_t*)dx->take(msr_dense::S_N, std::max<size_t>(nq, 1) * 4);
    int32_t* d_self = nullptr;
    bool ok = s.d_Q && s.d_S && d_ord && d_sf && d_n;
    if (ok && self_ord)
        ok = (d_self = (int32_t*)dx->take(msr_dense::S_SELF, std::max<size_t>(nq, 1) * 4)) != nullptr &&
             hipMemcpyAsync(d_self, self_ord, (size_t)nq * 4, hipMemcpyHostToDevice, d->stream) == hipSuccess;
    if (ok && nq) ok = upload_query_rows(dx, s.d_Q, q, (size_t)nq, nq_pad, d->stream);
    s.ok = ok;
    fill_score_args(s.sa, s.b, k);
    s.sa.part = nullptr;
    HybridArgs& ha = s.ha;
    ha.dkeys = s.d_S;
    ha.ld = ld;
    ha.self_ord = d_self;
    ha.depth = (uint32_t)depth;
    ha.k = (uint32_t)k;
    ha.w_dense = alpha;
    ha.w_sparse = 1.0f - alpha;
    ha.out_ord = d_ord;
    ha.out_score = d_sf;
    ha.out_n = d_n;
    return MSR_OK;
}

// the result lists of a hybrid call back to the host
static int hybrid_download(const HybridArgs& ha, int nq, int k, uint32_t* out_ord, float* out_score, int32_t* out_n) {
    if (nq && (hipMemcpy(out_ord, ha.out_ord, (size_t)nq * k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(out_score, ha.out_score, (size_t)nq * k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
               hipMemcpy(out_n, ha.out_n, (size_t)nq * 4, hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("download failed in msr_hybrid_search");
        return MSR_E_HIP;
    }
    return MSR_OK;
}

// hybrid_tiles<MODE> at the tile's launch shape (1024 candidate keys: waves_rest); only the `light` shapes have one
template <int MODE>
static void launch_hybrid_tiles(uint32_t tile_docs, dim3 grid, hipStream_t st, const ScoreArgs& sa, const HybridArgs& ha) {
    with_tile_shape(tile_docs, [&](auto sh) {
        using S = decltype(sh);
        if constexpr (S::light)
            hipLaunchKernelGGL((hybrid_tiles<S::docs, S::threads, S::loads, S::waves_rest, MODE>), grid, dim3(S::threads), 0, st, sa, ha);
    });
}

// The fused path of msr_hybrid_search (single-tile indexes, k <= 64): per chunk of queries (normally ONE chunk) a GEMM
// launch on the ordinal-permuted passage matrix, then hybrid_tiles. ms = {fused scoring + selection + fusion kernel, dense GEMM, 0, 0}.
static int hybrid_search_fused(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                               const void* q, int nq, int depth, int k, float alpha, uint32_t flags,
                               const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score,
                               int32_t* out_n, float ms[4]) {
    DeviceIndex* d = ix->dev;
    const IndexHeader* h = ix->host.h;
    const uint64_t n = h->n_docs;
    HIP_TRY(hipSetDevice(d->device));
    const uint32_t nt_threads = tile_threads(h->tile_docs);
    const uint64_t ld = (n + 4 * nt_threads - 1) / (4 * nt_threads) * (4 * nt_threads);  // whole select rounds
    const uint64_t n_cover = std::min<uint64_t>(dx->n_pad, (n + 255) / 256 * 256);
    const uint32_t gb = hybrid_gemm_block(dx);  // 256 x 256 fp16 blocks, 128 x 128 f32 blocks
    const uint32_t col_blocks = (uint32_t)(n_cover / gb);
    const uint32_t nq_pad = (uint32_t)((nq + gb - 1) / gb * gb);
    // queries per chunk: whole rounds of the chip's 256 CUs worth of GEMM blocks, score rows <= ~160 MB so
    // that hybrid_tiles finds its row in the Infinity Cache (the row load is a dependent fetch at the start of the
    // epilogue: from HBM the same kernel measured 1.66 ms instead of 1.30 ms per 25 010 queries)
    uint64_t row_blocks = std::max<uint64_t>(1, kHybridChunkBytes / (ld * 4 * gb));
    if (col_blocks && row_blocks * col_blocks >= 256) row_blocks = row_blocks * col_blocks / 256 * 256 / col_blocks;
    const uint32_t qc = (uint32_t)std::min<uint64_t>(row_blocks * gb, std::max<uint32_t>(nq_pad, gb));
    HybridSetup s;
    if (int rc0 = hybrid_setup(ix, dx, q_ptr, q_term, q_w, q, nq, k, depth, k, alpha, flags, row2ord, self_ord, ld,
                               (size_t)qc * ld * 4, s))
        return rc0;
    ScoreArgs& sa = s.sa;
    const HybridArgs& ha = s.ha;
    int rc = MSR_OK;
    if (!s.ok) {
        set_error("device allocation or query upload failed in msr_hybrid_search (%u queries per chunk)", qc);
        rc = MSR_E_NOMEM;
    }
    std::vector<hipEvent_t> ev;
    for (uint32_t q0 = 0; q0 < (uint32_t)nq && rc == MSR_OK; q0 += qc) {
        const uint32_t qn = std::min<uint32_t>(qc, (uint32_t)nq - q0);
        const uint32_t qn_pad = (qn + gb - 1) / gb * gb;
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        for (auto& x : e) {
            if (hipEventCreate(&x) != hipSuccess) rc = MSR_E_HIP;
            ev.push_back(x);
        }
        if (rc != MSR_OK) {
            set_error("hipEventCreate failed");
            break;
        }
        (void)hipEventRecord(e[0], d->stream);
        rc = launch_hybrid_gemm(dx, s.d_Q + (size_t)q0 * dense_row_bytes(dx), s.d_S, qn, qn_pad, n_cover, ld, d->stream);
        if (rc != MSR_OK) break;
        (void)hipEventRecord(e[1], d->stream);
        sa.q0 = q0;
        sa.qn = qn;
        launch_hybrid_tiles<0>(h->tile_docs, dim3(qn), d->stream, sa, ha);
        if (hipGetLastError() != hipSuccess) {
            set_error("hybrid_tiles launch failed: %s", hipGetErrorString(hipGetLastError()));
            rc = MSR_E_HIP;
            break;
        }
        (void)hipEventRecord(e[2], d->stream);
    }
    if (rc == MSR_OK && hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("hybrid kernels failed: %s", hipGetErrorString(hipGetLastError()));
        rc = MSR_E_HIP;
    }
    float t_gemm = 0, t_fused = 0;
    if (rc == MSR_OK) {
        for (size_t i = 0; i + 2 < ev.size(); i += 3) {
            float a = 0, c = 0;
            (void)hipEventElapsedTime(&a, ev[i], ev[i + 1]);
            (void)hipEventElapsedTime(&c, ev[i + 1], ev[i + 2]);
            t_gemm += a;
            t_fused += c;
        }
        rc = hybrid_download(ha, nq, k, out_ord, out_score, out_n);
    }
    if (ms) {
        ms[0] = t_fused;
        ms[1] = t_gemm;
        ms[2] = 0.f;
        ms[3] = 0.f;
    }
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    // (the scratch stays with the dense handle for the next call)
    batch_free(s.b);
    return rc;
}

// Candidate quota of a tile that holds `tile_docs` of the corpus's `n` docs: its expected share of a depth list plus
// five standard deviations (docs are numbered by id string, so a tile's share of any query's best docs is a draw without
// replacement) plus a constant; never more than the depth. A query for which some tile needed more is repeated with
// quota = depth by the caller, so the result never depends on this number.
static uint32_t tile_quota(uint64_t tile_docs, uint64_t n, uint32_t depth) {
    const char* env = getenv("MSR_HYBRID_QUOTA");  // diagnostic / tests (read per call: a test flips it)
    const long forced = env ? atol(env) : 0;
    if (forced > 0) return (uint32_t)std::min<long>(forced, depth);
    if (n == 0 || tile_docs >= n) return depth;
    const double share = (double)tile_docs / (double)n, mean = depth * share;
    const double q = mean + 5.0 * std::sqrt(mean * (1.0 - share)) + 16.0;
    return (uint32_t)std::min<double>(depth, std::ceil(q));
}

// Multi-tile indexes (and k > 64 on one tile): per chunk of queries a GEMM launch on the ordinal-permuted passage matrix,
// hybrid_tiles<MODE 1> over (query, tile) and hybrid_fuse_query over the queries; flagged queries (normally none) are
// repeated with quota = depth. ms = {candidate kernel, dense GEMM, 0, fusion kernel}.
// un != null (msr_hybrid_search_union): k = 2 x depth is the row length, hybrid_fuse_query<UNION> keeps the whole union and fills
// the optional arrays that un names (host pointers, null = not wanted: neither allocated, written nor downloaded).
// un->resident != null (msr_hybrid_sweep): every side array and the exact sparse extremes are computed, NOTHING is downloaded
// (out_ord / out_score / out_n may be null) and *resident receives the device pointers, which stay valid in the dense
// handle's scratch until its next call.
struct UnionResident {
    UnionOut uo;
    const uint32_t* ord;  // [nq][2 x depth] members by the fused score of the pass's alpha
    const int32_t* n;     // [nq]
};
struct UnionHost {
    uint8_t* src;
    uint32_t* sparse;
    float* dense;
    float* range;
    UnionResident* resident = nullptr;
};

static int hybrid_search_multitile(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term,
                                   const int32_t* q_w, const void* q, int nq, int depth, int k, float alpha,
                                   uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord,
                                   float* out_score, int32_t* out_n, float ms[4], const UnionHost* un = nullptr) {
    DeviceIndex* d = ix->dev;
    const IndexHeader* h = ix->host.h;
    const uint64_t n = h->n_docs;
    const uint32_t tile = h->tile_docs, n_tiles = h->n_tiles;
    HIP_TRY(hipSetDevice(d->device));
    const uint64_t ld = (uint64_t)n_tiles * tile;  // a query's score row: tile t starts at column t * tile
    const uint64_t n_cover = std::min<uint64_t>(dx->n_pad, (n + 255) / 256 * 256);
    const uint32_t gb = hybrid_gemm_block(dx);  // 256 x 256 fp16 blocks, 128 x 128 f32 blocks
    const uint32_t col_blocks = (uint32_t)(n_cover / gb);
    const uint32_t nq_pad = (uint32_t)((nq + gb - 1) / gb * gb);
    // queries per chunk: score rows of ~160 MB (they are read back out of the Infinity Cache), whole rounds of the
    // chip's 256 CUs worth of GEMM blocks (the bytes that travel are the n_cover written columns of a row, not its
    // padded stride). Among the chunk sizes that fit, the one whose GEMM grid fills its last round of 256 CUs best:
    // 2 x 98 blocks leave a quarter of the chip idle, 5 x 98 = 490 fill 1.91 rounds
    const uint64_t rb_max = std::max<uint64_t>(1, kHybridChunkBytes / (std::max<uint64_t>(n_cover, gb) * 4 * gb));
    const uint64_t row_blocks = pick_row_blocks(col_blocks, rb_max, nq_pad / gb);
    const uint32_t qc = (uint32_t)std::min<uint64_t>(row_blocks * gb, std::max<uint32_t>(nq_pad, gb));
    const uint64_t last_docs = n - (uint64_t)(n_tiles - 1) * tile;
    const uint32_t quota_full = n_tiles > 1 ? tile_quota(tile, n, (uint32_t)depth) : tile_quota(n, n, (uint32_t)depth);
    const uint32_t quota_last = n_tiles > 1 ? std::min(quota_full, tile_quota(last_docs, n, (uint32_t)depth)) : quota_full;
    // candidate slots: a chunk of the first round (qc rows x quota_full) or at least ONE row of the second (depth)
    const size_t per_tile_row = (size_t)n_tiles;
    // record slots (a tile's union of two candidate sets: 2 x quota): a chunk of the first round or at least ONE row of the second
    const size_t cand_slots = 2 * std::max<size_t>((size_t)qc * per_tile_row * quota_full, per_tile_row * (size_t)depth);
    HybridSetup s;  // (a batch for k = 1: only its query arrays are used)
    if (int rc0 = hybrid_setup(ix, dx, q_ptr, q_term, q_w, q, nq, 1, depth, k, alpha, flags, row2ord, self_ord, ld,
                               (size_t)qc * ld * 4, s))
        return rc0;
    ScoreArgs& sa = s.sa;
    HybridArgs& ha = s.ha;
    uint32_t* d_rec = (uint32_t*)dx->take(msr_dense::S_CS, cand_slots * 12);  // ordinals | sparse scores | dense keys
    uint4* d_meta = (uint4*)dx->take(msr_dense::S_META, std::max<size_t>((size_t)qc * per_tile_row * 2 * 16, 32));
    uint32_t* d_flags = (uint32_t*)dx->take(msr_dense::S_FLAGS, std::max<size_t>(nq, 1) * 4);
    uint32_t* d_qlist = (uint32_t*)dx->take(msr_dense::S_QLIST, std::max<size_t>(nq, 1) * 4);
    bool ok = s.ok && d_rec && d_meta && d_flags && d_qlist;
    UnionOut uo = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t per_union = std::max<size_t>((size_t)nq * k, 1);  // (un: k = 2 x depth)
    const bool resident = un && un->resident;
    if (un) {
        if (resident) ok = (uo.ext = (uint32_t*)dx->take(msr_dense::S_UEXT, std::max<size_t>(nq, 1) * 8)) != nullptr && ok;
        if (un->src || resident) ok = (uo.src = (uint8_t*)dx->take(msr_dense::S_USRC, per_union)) != nullptr && ok;
        if (un->sparse || resident) ok = (uo.sparse = (uint32_t*)dx->take(msr_dense::S_USPARSE, per_union * 4)) != nullptr && ok;
        if (un->dense || resident) ok = (uo.dense = (float*)dx->take(msr_dense::S_UDENSE, per_union * 4)) != nullptr && ok;
        if (un->range || resident) ok = (uo.range = (float*)dx->take(msr_dense::S_URANGE, std::max<size_t>(nq, 1) * 16)) != nullptr && ok;
    }
    int rc = MSR_OK;
    if (!ok) {
        set_error("device allocation or query upload failed in %s (%u queries per chunk, %u tiles)",
                  un ? "msr_hybrid_search_union" : "msr_hybrid_search", qc, n_tiles);
        rc = MSR_E_NOMEM;
    }
    ha.qlist = nullptr;
    ha.rec_ord = d_rec;
    ha.rec_s = d_rec + cand_slots;
    ha.rec_d = d_rec + 2 * cand_slots;
    ha.tile_meta = d_meta;
    ha.n_tiles = n_tiles;
    ha.stride = 2 * quota_full;
    ha.quota_full = quota_full;
    ha.quota_last = quota_last;
    ha.flags = d_flags;
    // one pass of the three kernels over `rows` launch rows (queries q0 .. or the listed ones), dense rows from d_Qrows
    auto launch_rows = [&](const uint8_t* d_Qrows, uint32_t rows, uint32_t q0, hipEvent_t* e) -> int {
        const uint32_t rows_pad = (rows + gb - 1) / gb * gb;
        if (e) (void)hipEventRecord(e[0], d->stream);
        int r2 = launch_hybrid_gemm(dx, d_Qrows, s.d_S, rows, rows_pad, n_cover, ld, d->stream);
        if (r2 != MSR_OK) return r2;
        if (e) (void)hipEventRecord(e[1], d->stream);
        sa.q0 = q0;
        sa.qn = rows;
        for (uint32_t t0 = 0; t0 < n_tiles; t0 += kMaxGridY) {  // (grid y limit; tile_l = blockIdx.y needs t0 == 0)
            if (t0) {
                set_error("msr_hybrid_search: more than %u tiles", kMaxGridY);
                return MSR_E_RANGE;
            }
            const dim3 grid(rows, n_tiles);
            launch_hybrid_tiles<1>(tile, grid, d->stream, sa, ha);
        }
        if (hipGetLastError() != hipSuccess) {
            set_error("hybrid_tiles launch failed: %s", hipGetErrorString(hipGetLastError()));
            return MSR_E_HIP;
        }
        if (e) (void)hipEventRecord(e[2], d->stream);
        // (a query's records stay in registers while they fit: 16 per thread)
        const bool small = (uint64_t)ha.n_tiles * ha.stride <= 256u * 16u;
        if (un && small)
            hipLaunchKernelGGL((hybrid_fuse_query<256, 16, true>), dim3(rows), dim3(256), 0, d->stream, ha, q0, uo);
        else if (un)
            hipLaunchKernelGGL((hybrid_fuse_query<512, 16, true>), dim3(rows), dim3(512), 0, d->stream, ha, q0, uo);
        else if (small)
            hipLaunchKernelGGL((hybrid_fuse_query<256, 16>), dim3(rows), dim3(256), 0, d->stream, ha, q0, uo);
        else
            hipLaunchKernelGGL((hybrid_fuse_query<512, 16>), dim3(rows), dim3(512), 0, d->stream, ha, q0, uo);
        if (hipGetLastError() != hipSuccess) {
            set_error("hybrid_fuse_query launch failed: %s", hipGetErrorString(hipGetLastError()));
            return MSR_E_HIP;
        }
        if (e) (void)hipEventRecord(e[3], d->stream);
        return MSR_OK;
    };
    std::vector<hipEvent_t> ev;
    auto four_events = [&]() -> hipEvent_t* {
        const size_t at = ev.size();
        bool all = true;
        for (int i = 0; i < 4; ++i) {
            ev.push_back(d->borrow_event());
            all = all && ev.back();
        }
        return all ? ev.data() + at : nullptr;
    };
    ev.reserve(4 * ((size_t)nq / std::max<uint32_t>(qc, 1) + 4) + 64);  // (pointers into ev stay valid)
    for (uint32_t q0 = 0; q0 < (uint32_t)nq && rc == MSR_OK; q0 += qc) {
        const uint32_t qn = std::min<uint32_t>(qc, (uint32_t)nq - q0);
        hipEvent_t* e = four_events();
        if (!e) {
            set_error("hipEventCreate failed");
            rc = MSR_E_HIP;
            break;
        }
        rc = launch_rows(s.d_Q + (size_t)q0 * dense_row_bytes(dx), qn, q0, e);
    }
    std::vector<uint32_t> hflags((size_t)nq, 0);
    if (rc == MSR_OK && nq &&
        (hipMemcpyAsync(hflags.data(), d_flags, (size_t)nq * 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
         hipStreamSynchronize(d->stream) != hipSuccess)) {
        set_error("hybrid kernels failed: %s", hipGetErrorString(hipGetLastError()));
        rc = MSR_E_HIP;
    }
    // ---- second round (normally empty): the flagged queries again, every tile emitting its own top-depth
    std::vector<uint32_t> redo;
    for (int i = 0; i < nq && rc == MSR_OK; ++i)
        if (hflags[(size_t)i]) redo.push_back((uint32_t)i);
    if (rc == MSR_OK && !redo.empty()) {
        const uint32_t rows_cap = (uint32_t)std::min<size_t>(std::min<size_t>(cand_slots / (2 * per_tile_row * (size_t)depth), qc), redo.size());
        const size_t h_row = (size_t)dx->h * (dx->f32 ? 4 : 2);  // bytes per row of the caller's query matrix
        std::vector<uint8_t> qrows((size_t)rows_cap * h_row);
        ha.quota_full = ha.quota_last = (uint32_t)depth;
        ha.stride = 2 * (uint32_t)depth;
        ha.qlist = d_qlist;
        for (size_t at = 0; at < redo.size() && rc == MSR_OK; at += rows_cap) {
            const uint32_t rows = (uint32_t)std::min<size_t>(rows_cap, redo.size() - at);
            const uint32_t rows_pad = (rows + gb - 1) / gb * gb;
            for (uint32_t r = 0; r < rows; ++r)
                memcpy(qrows.data() + (size_t)r * h_row, (const uint8_t*)q + (size_t)redo[at + r] * h_row, h_row);
            // (d_Q's first rows are reused: the first round is over)
            ok = upload_query_rows(dx, s.d_Q, qrows.data(), rows, rows_pad, d->stream) &&
                 hipMemcpyAsync(d_qlist, redo.data() + at, (size_t)rows * 4, hipMemcpyHostToDevice, d->stream) == hipSuccess;
            if (!ok) {
                set_error("upload failed in the second round of msr_hybrid_search");
                rc = MSR_E_HIP;
                break;
            }
            hipEvent_t* e = ev.size() + 4 <= ev.capacity() ? four_events() : nullptr;
            rc = launch_rows(s.d_Q, rows, 0, e);
            if (rc == MSR_OK && hipStreamSynchronize(d->stream) != hipSuccess) {  // (qrows / redo are re-filled next)
                set_error("hybrid kernels failed in the second round: %s", hipGetErrorString(hipGetLastError()));
                rc = MSR_E_HIP;
            }
        }
        if (rc == MSR_OK) {  // with quota = depth every list is complete by construction
            (void)hipMemcpy(hflags.data(), d_flags, (size_t)nq * 4, hipMemcpyDeviceToHost);
            for (uint32_t i : redo)
                if (hflags[i]) {
                    set_error("internal error: query %u still incomplete after the second round", i);
                    rc = MSR_E_HIP;
                    break;
                }
        }
    }
    float t_gemm = 0, t_cand = 0, t_fuse = 0;
    if (rc == MSR_OK) {
        for (size_t i = 0; i + 3 < ev.size(); i += 4) {
            float a = 0, c = 0, f = 0;
            (void)hipEventElapsedTime(&a, ev[i], ev[i + 1]);
            (void)hipEventElapsedTime(&c, ev[i + 1], ev[i + 2]);
            (void)hipEventElapsedTime(&f, ev[i + 2], ev[i + 3]);
            t_gemm += a;
            t_cand += c;
            t_fuse += f;
        }
        if (resident) {
            un->resident->uo = uo;
            un->resident->ord = ha.out_ord;
            un->resident->n = ha.out_n;
        } else {
            rc = hybrid_download(ha, nq, k, out_ord, out_score, out_n);
        }
        if (rc == MSR_OK && un && !resident && nq &&
            ((un->src && hipMemcpy(un->src, uo.src, (size_t)nq * k, hipMemcpyDeviceToHost) != hipSuccess) ||
             (un->sparse && hipMemcpy(un->sparse, uo.sparse, (size_t)nq * k * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
             (un->dense && hipMemcpy(un->dense, uo.dense, (size_t)nq * k * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
             (un->range && hipMemcpy(un->range, uo.range, (size_t)nq * 16, hipMemcpyDeviceToHost) != hipSuccess))) {
            set_error("download of the union's side arrays failed in msr_hybrid_search_union");
            rc = MSR_E_HIP;
        }
    }
    if (ms) {
        ms[0] = t_cand;
        ms[1] = t_gemm;
        ms[2] = 0.f;
        ms[3] = t_fuse;
    }
    for (hipEvent_t x : ev) d->return_event(x);
    batch_free(s.b);
    return rc;
}

// msr_hybrid_search and msr_hybrid_search_f32 after their precision check: q is [nq][h] in the handle's precision
static int hybrid_search_impl(const char* fn, msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term,
                              const int32_t* q_w, const void* q, int nq, int depth, int k, float alpha, uint32_t flags,
                              const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score,
                              int32_t* out_n, float ms[4]) {
    if (!ix || !dx || !row2ord || !out_ord || !out_score || !out_n || nq < 0 || (nq && !q)) {
        set_error("%s: bad argument", fn);
        return MSR_E_INVAL;
    }
    if (!ix->dev) {
        set_error("index handle has no HIP device bound; there is no CPU scoring path");
        return MSR_E_NODEVICE;
    }
    if (ix->dev->device != dx->device) {
        set_error("the sparse and the dense index live on different devices");
        return MSR_E_INVAL;
    }
    if (depth < 1 || depth > MSR_KMAX || k < 1 || k > MSR_KMAX) {
        set_error("depth and k must be in [1, %d]", MSR_KMAX);
        return MSR_E_RANGE;
    }
    if (dx->n != ix->host.h->n_docs) {
        set_error("the dense index holds %llu rows but the sparse index %llu docs", (unsigned long long)dx->n,
                  (unsigned long long)ix->host.h->n_docs);
        return MSR_E_INVAL;
    }
    DeviceIndex* d = ix->dev;
    const IndexHeader* h = ix->host.h;
    static const bool no_fused = getenv("MSR_NO_FUSED_HYBRID") != nullptr;  // diagnostic: force the list-based path
    // (permute_rows moves uint4: an fp16 row needs h % 8 == 0; an f32 row of hp floats always qualifies)
    const bool rows_ok = dx->f32 || dx->h % 8 == 0;
    if (!no_fused && h->n_tiles == 1 && ix->shard_ntiles == 1 && ix->term_nshards == 0 && k <= 64 && rows_ok &&
        hybrid_tile(h->tile_docs))
        return hybrid_search_fused(ix, dx, q_ptr, q_term, q_w, q, nq, depth, k, alpha, flags, row2ord, self_ord,
                                   out_ord, out_score, out_n, ms);
    if (!no_fused && ix->shard_ntiles == h->n_tiles && ix->term_nshards == 0 && rows_ok && h->n_tiles <= kMaxGridY &&
        hybrid_tile(h->tile_docs))
        return hybrid_search_multitile(ix, dx, q_ptr, q_term, q_w, q, nq, depth, k, alpha, flags, row2ord, self_ord,
                                       out_ord, out_score, out_n, ms);
    msr_batch* b = nullptr;
    int rc = msr_batch_create(ix, q_ptr, q_term, q_w, nq, depth, flags, &b);
    if (rc != MSR_OK) return rc;
    uint32_t *d_didx = nullptr, *d_dkey = nullptr, *d_map = nullptr, *d_ord = nullptr, *d_su = nullptr;
    int32_t *d_dn = nullptr, *d_self = nullptr, *d_n = nullptr;
    float* d_sf = nullptr;
    uint64_t* d_part = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const uint32_t ftile = h->n_docs <= 4096 ? 4096 : 8192;
    const uint32_t ftiles = (uint32_t)std::max<uint64_t>((h->n_docs + ftile - 1) / ftile, 1);
    const size_t per = std::max<size_t>((size_t)nq * depth, 1), perk = std::max<size_t>((size_t)nq * k, 1);
    bool ok = hipSetDevice(d->device) == hipSuccess && hipMalloc(&d_didx, per * 4) == hipSuccess &&
              hipMalloc(&d_dkey, per * 4) == hipSuccess && hipMalloc(&d_dn, std::max<size_t>(nq, 1) * 4) == hipSuccess &&
              hipMalloc(&d_map, std::max<size_t>(h->n_docs, 1) * 4) == hipSuccess &&
              hipMalloc(&d_part, (size_t)ftiles * perk * 8) == hipSuccess && hipMalloc(&d_ord, perk * 4) == hipSuccess &&
              hipMalloc(&d_su, perk * 4) == hipSuccess && hipMalloc(&d_sf, perk * 4) == hipSuccess &&
              hipMalloc(&d_n, std::max<size_t>(nq, 1) * 4) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
              hipEventCreate(&e1) == hipSuccess &&
              hipMemcpy(d_map, row2ord, (size_t)h->n_docs * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && self_ord)
        ok = hipMalloc(&d_self, std::max<size_t>(nq, 1) * 4) == hipSuccess &&
             hipMemcpy(d_self, self_ord, (size_t)nq * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        set_error("device allocation failed in msr_hybrid_search");
        rc = MSR_E_NOMEM;
    }
    float t_gemm = 0, t_sel = 0, t_sparse = 0, t_merge = 0, t_fuse = 0;
    // fuse_tiles takes both top-depth lists as SETS (min, max, membership): single-tile indexes skip the ranking
    b->unsorted_ok = true;
    if (rc == MSR_OK) rc = batch_search_local(b, depth, false);  // sparse top-depth keys -> b->d_keys
    if (rc == MSR_OK) rc = dense_search_impl(dx, q, nq, depth, d_didx, d_dkey, d_dn, &t_gemm, &t_sel, true, true);
    if (rc == MSR_OK) {
        (void)hipEventRecord(e0, d->stream);
        FuseArgs fa;
        fa.s_keys = b->d_keys;
        fa.d_idx = d_didx;
        fa.d_key = d_dkey;
        fa.d_n = d_dn;
        fa.row2ord = d_map;
        fa.self_ord = d_self;
        fa.part = d_part;
        fa.n_docs = h->n_docs;
        fa.nq = (uint32_t)nq;
        fa.depth = (uint32_t)depth;
        fa.k = (uint32_t)k;
        fa.w_dense = alpha;
        fa.w_sparse = 1.0f - alpha;
        if (nq)
            with_tile_shape(ftile, [&](auto sh) {
                using S = decltype(sh);
                if constexpr (S::light)
                    hipLaunchKernelGGL((fuse_tiles<S::docs, S::threads, 1024>), dim3(ftiles * (uint32_t)nq), dim3(S::threads), 0,
                                       d->stream, fa);
            });
        MergeArgs ma;
        ma.lists = d_part;
        ma.list_stride = (uint64_t)nq * k;
        ma.n_lists = ftiles;
        ma.nq = (uint32_t)nq;
        ma.k = (uint32_t)k;
        ma.out_keys = nullptr;
        ma.out_ord = d_ord;
        ma.out_score_u32 = d_su;
        ma.out_score = d_sf;
        ma.out_n = d_n;
        rc = launch_merge(d->stream, ma);
        (void)hipEventRecord(e1, d->stream);
    }
    if (rc == MSR_OK && hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("hybrid kernels failed: %s", hipGetErrorString(hipGetLastError()));
        rc = MSR_E_HIP;
    }
    if (rc == MSR_OK) {
        (void)msr_batch_kernel_ms(b, &t_sparse, &t_merge);
        (void)hipEventElapsedTime(&t_fuse, e0, e1);
        // out_score: the fused f32 score is carried as an order-preserving key in the u32 score slot
        std::vector<uint32_t> keys((size_t)nq * k);
        bool c = (!nq) || (hipMemcpy(out_ord, d_ord, (size_t)nq * k * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                           hipMemcpy(keys.data(), d_su, (size_t)nq * k * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                           hipMemcpy(out_n, d_n, (size_t)nq * 4, hipMemcpyDeviceToHost) == hipSuccess);
        if (!c) {
            set_error("download failed in msr_hybrid_search");
            rc = MSR_E_HIP;
        } else {
            for (size_t i = 0; i < keys.size(); ++i) {
                const uint32_t key = keys[i];
                uint32_t bits = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
                float f;
                memcpy(&f, &bits, 4);
                out_score[i] = key ? f : 0.f;
            }
        }
    }
    if (ms) {
        ms[0] = t_sparse + t_merge;
        ms[1] = t_gemm;
        ms[2] = t_sel;
        ms[3] = t_fuse;
    }
    void* ptrs[] = {d_didx, d_dkey, d_dn, d_map, d_self, d_part, d_ord, d_su, d_sf, d_n};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    batch_free(b);
    return rc;
}

extern "C" {

int msr_hybrid_search(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                      const uint16_t* q_fp16, int nq, int depth, int k, float alpha, uint32_t flags,
                      const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score, int32_t* out_n,
                      float ms[4]) {
    if (dx && dx->f32) {
        set_error("msr_hybrid_search: the dense handle holds f32 rows (msr_dense_open_f32); search it with "
                  "msr_hybrid_search_f32, or open an fp16 handle (msr_dense_open)");
        return MSR_E_INVAL;
    }
    return hybrid_search_impl("msr_hybrid_search", ix, dx, q_ptr, q_term, q_w, q_fp16, nq, depth, k, alpha, flags, row2ord,
                              self_ord, out_ord, out_score, out_n, ms);
}

int msr_hybrid_search_f32(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                          const float* q, int nq, int depth, int k, float alpha, uint32_t flags, const uint32_t* row2ord,
                          const int32_t* self_ord, uint32_t* out_ord, float* out_score, int32_t* out_n, float ms[4]) {
    if (dx && !dx->f32) {
        set_error("msr_hybrid_search_f32: the dense handle holds fp16 rows (msr_dense_open); search it with "
                  "msr_hybrid_search, or open an f32 handle (msr_dense_open_f32)");
        return MSR_E_INVAL;
    }
    return hybrid_search_impl("msr_hybrid_search_f32", ix, dx, q_ptr, q_term, q_w, q, nq, depth, k, alpha, flags, row2ord,
                              self_ord, out_ord, out_score, out_n, ms);
}

int msr_hybrid_search_union(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                            const void* q, int q_is_f32, int nq, int depth, float alpha, uint32_t flags,
                            const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score,
                            int32_t* out_n, uint8_t* out_src, uint32_t* out_sparse_u32, float* out_dense, float* out_range,
                            float ms[4]) {
    if (!ix || !dx || !row2ord || !out_ord || !out_score || !out_n || nq < 0 || (nq && !q)) {
        set_error("msr_hybrid_search_union: bad argument");
        return MSR_E_INVAL;
    }
    if (int rc0 = dense_precision_check("msr_hybrid_search_union", dx, q_is_f32)) return rc0;
    if (!ix->dev) {
        set_error("index handle has no HIP device bound; there is no CPU scoring path");
        return MSR_E_NODEVICE;
    }
    if (ix->dev->device != dx->device) {
        set_error("the sparse and the dense index live on different devices");
        return MSR_E_INVAL;
    }
    if (depth < 1 || depth > MSR_KMAX) {
        set_error("msr_hybrid_search_union: depth must be in [1, %d]", MSR_KMAX);
        return MSR_E_RANGE;
    }
    const IndexHeader* h = ix->host.h;
    if (dx->n != h->n_docs) {
        set_error("the dense index holds %llu rows but the sparse index %llu docs", (unsigned long long)dx->n,
                  (unsigned long long)h->n_docs);
        return MSR_E_INVAL;
    }
    // the handles the candidate path of hybrid_search_impl takes; there is no list-based union
    const char* why = nullptr;
    if (ix->term_nshards != 0) why = "a term-range shard handle";
    else if (ix->shard_ntiles != h->n_tiles) why = "a doc-range shard handle";
    else if (!hybrid_tile(h->tile_docs)) why = "a tile size other than 4096 / 8192 docs";
    else if (h->n_tiles > kMaxGridY) why = "more tiles than one launch holds";
    else if (!dx->f32 && dx->h % 8 != 0) why = "an fp16 dense dimension that is not a multiple of 8";
    if (why) {
        set_error("msr_hybrid_search_union: %s is not supported (tile_docs %u, %u of %u tiles resident): the whole union "
                  "needs a whole-index handle with 4096- or 8192-doc tiles", why, h->tile_docs, ix->shard_ntiles, h->n_tiles);
        return MSR_E_INVAL;
    }
    const UnionHost un = {out_src, out_sparse_u32, out_dense, out_range};
    return hybrid_search_multitile(ix, dx, q_ptr, q_term, q_w, q, nq, depth, 2 * depth, alpha, flags, row2ord, self_ord,
                                   out_ord, out_score, out_n, ms, &un);
}

// Device staging of one fuse_sweep launch's [alphas][nq][k] lists (ordinals + scores): the bound of the deep calls. A
// launch takes at least one alpha, so a batch whose ONE alpha is larger is staged whole (the union pass's own arrays of
// that batch are larger still).
constexpr size_t kSweepStageBytes = 256ull << 20;

int msr_hybrid_sweep(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                     const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas, int n_alphas,
                     uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord,
                     float* out_score, int32_t* out_n, float ms[6]) {
    static_assert(MSR_SWEEP_MAX_ALPHAS == kSweepMaxAlphas, "the kernel's alpha array");
    if (ms)
        for (int i = 0; i < 6; ++i) ms[i] = 0.f;
    if (!ix || !dx || !q_ptr || !row2ord || !alphas || !out_ord || !out_score || !out_n || nq < 0 || (nq && !q)) {
        set_error("msr_hybrid_sweep: bad argument");
        return MSR_E_INVAL;
    }
    if (int rc0 = dense_precision_check("msr_hybrid_sweep", dx, q_is_f32)) return rc0;
    const IndexHeader* h = ix->host.h;
    if (dx->n != h->n_docs) {
        set_error("the dense index holds %llu rows but the sparse index %llu docs", (unsigned long long)dx->n,
                  (unsigned long long)h->n_docs);
        return MSR_E_INVAL;
    }
    // the handles of msr_hybrid_search_union: the sweep consumes that pass's resident union
    const char* why = nullptr;
    if (ix->term_nshards != 0) why = "a term-range shard handle";
    else if (ix->shard_ntiles != h->n_tiles) why = "a doc-range shard handle";
    else if (!hybrid_tile(h->tile_docs)) why = "a tile size other than 4096 / 8192 docs";
    else if (h->n_tiles > kMaxGridY) why = "more tiles than one launch holds";
    else if (!dx->f32 && dx->h % 8 != 0) why = "an fp16 dense dimension that is not a multiple of 8";
    if (why) {
        set_error("msr_hybrid_sweep: %s is not supported (tile_docs %u, %u of %u tiles resident): the sweep needs a "
                  "whole-index handle with 4096- or 8192-doc tiles", why, h->tile_docs, ix->shard_ntiles, h->n_tiles);
        return MSR_E_INVAL;
    }
    for (int i = 0; i < std::min(n_alphas, (int)MSR_SWEEP_MAX_ALPHAS); ++i)
        if (!std::isfinite(alphas[i])) {
            set_error("msr_hybrid_sweep: alphas[%d] is not finite", i);
            return MSR_E_INVAL;
        }
    if (depth < 1 || depth > MSR_KMAX) {
        set_error("msr_hybrid_sweep: depth must be in [1, %d] (got %d)", MSR_KMAX, depth);
        return MSR_E_RANGE;
    }
    if (k < 1 || k > 2 * depth) {
        set_error("msr_hybrid_sweep: k must be in [1, 2 x depth = %d] (got %d)", 2 * depth, k);
        return MSR_E_RANGE;
    }
    if (n_alphas < 1 || n_alphas > MSR_SWEEP_MAX_ALPHAS) {
        set_error("msr_hybrid_sweep: n_alphas must be in [1, %d] (got %d)", MSR_SWEEP_MAX_ALPHAS, n_alphas);
        return MSR_E_RANGE;
    }
    if (!ix->dev) {
        set_error("index handle has no HIP device bound; there is no CPU scoring path");
        return MSR_E_NODEVICE;
    }
    if (int rc0 = dense_device_check("msr_hybrid_sweep", dx)) return rc0;
    if (ix->dev->device != dx->device) {
        set_error("the sparse and the dense index live on different devices");
        return MSR_E_INVAL;
    }
    if (nq == 0) return MSR_OK;
    // ---- one scoring: the union pass at any alpha; its outputs stay in the dense handle's scratch
    UnionResident res;
    const UnionHost un = {nullptr, nullptr, nullptr, nullptr, &res};
    if (int rc0 = hybrid_search_multitile(ix, dx, q_ptr, q_term, q_w, q, nq, depth, 2 * depth, alphas[0], flags, row2ord,
                                          self_ord, nullptr, nullptr, nullptr, ms, &un))
        return rc0;
    // ---- the sweep: alpha groups whose lists fit the staging bound; a group's [ga][nq][k] output is one contiguous piece
    // of the caller's [n_alphas][nq][k] arrays
    DeviceIndex* d = ix->dev;
    const size_t per_alpha = (size_t)nq * (size_t)k * 8;
    const uint32_t ga_max = (uint32_t)std::min<size_t>((size_t)n_alphas, std::max<size_t>(1, kSweepStageBytes / per_alpha));
    const size_t stage = (size_t)ga_max * (size_t)nq * (size_t)k;
    uint32_t* d_ord = (uint32_t*)dx->take(msr_dense::S_SW_ORD, stage * 4);
    float* d_sf = (float*)dx->take(msr_dense::S_SW_SF, stage * 4);
    int32_t* d_n = (int32_t*)dx->take(msr_dense::S_SW_N, (size_t)ga_max * (size_t)nq * 4);
    hipEvent_t e0 = d->borrow_event(), e1 = d->borrow_event();
    int rc = MSR_OK;
    if (!d_ord || !d_sf || !d_n || !e0 || !e1) {
        set_error("device allocation failed in msr_hybrid_sweep (%zu staged entries)", stage);
        rc = MSR_E_NOMEM;
    }
    SweepArgs sw;
    sw.u_ord = res.ord;
    sw.u_n = res.n;
    sw.src = res.uo.src;
    sw.sparse = res.uo.sparse;
    sw.dense = res.uo.dense;
    sw.range = res.uo.range;
    sw.ext = res.uo.ext;
    sw.w = 2 * (uint32_t)depth;
    sw.k = (uint32_t)k;
    sw.out_ord = d_ord;
    sw.out_score = d_sf;
    sw.out_n = d_n;
    sw.nq = (uint32_t)nq;
    float t_sweep = 0.f;
    uint32_t groups = 0;
    for (uint32_t a0 = 0; a0 < (uint32_t)n_alphas && rc == MSR_OK; a0 += ga_max, ++groups) {
        const uint32_t ga = std::min<uint32_t>(ga_max, (uint32_t)n_alphas - a0);
        for (int i = 0; i < kSweepMaxAlphas; ++i) sw.alpha[i] = (uint32_t)i < ga ? alphas[a0 + i] : 0.f;
        sw.n_alphas = ga;
        (void)hipEventRecord(e0, d->stream);
        hipLaunchKernelGGL(fuse_sweep, dim3((uint32_t)nq, (ga + kSweepAlphasPerWg - 1) / kSweepAlphasPerWg), dim3(kSweepThreads),
                           0, d->stream, sw);
        if (hipGetLastError() != hipSuccess) {
            set_error("fuse_sweep launch failed: %s", hipGetErrorString(hipGetLastError()));
            rc = MSR_E_HIP;
            break;
        }
        (void)hipEventRecord(e1, d->stream);
        if (hipStreamSynchronize(d->stream) != hipSuccess) {
            set_error("fuse_sweep failed: %s", hipGetErrorString(hipGetLastError()));
            rc = MSR_E_HIP;
            break;
        }
        const size_t at = (size_t)a0 * nq, rows = (size_t)ga * nq;
        if (hipMemcpy(out_ord + at * k, d_ord, rows * k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_score + at * k, d_sf, rows * k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_n + at, d_n, rows * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("download failed in msr_hybrid_sweep");
            rc = MSR_E_HIP;
            break;
        }
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        t_sweep += t;
    }
    if (e0) d->return_event(e0);
    if (e1) d->return_event(e1);
    if (ms) {
        ms[4] = t_sweep;
        ms[5] = (float)groups;
    }
    return rc;
}

// Key rows of one pass of msr_hybrid_deep: the LARGEST of its three row buffers (sparse scores and fused keys
// [qt][n_tiles x tile_docs], dense keys [qt][n_cover]) holds at most this many bytes, the rule of msr_search_deep and of the
// dense passes, with qt rounded down to whole row blocks of the hybrid GEMM (256 queries on fp16 handles, 128 on f32
// ones) and never below one block, so an index whose one block of rows is larger is still served, one block per pass.
constexpr uint64_t kHybridDeepPassBytes = 256ull << 20;

// The doc sets of an msr_hybrid_deep_filtered call as the caller passed them.
struct HybridDeepFilter {
    const uint32_t* set_bits;
    int n_sets;
    const int32_t* q_set;
};

}  // extern "C"

// msr_hybrid_deep (flt = null, 6 time slots) and msr_hybrid_deep_filtered (7 slots). Under a filter a pass with at least
// one filtered query launches score_dump_filtered in the place of the dump and mask_key_rows after the GEMM; every other
// launch, and every launch of a pass without a filtered query, is msr_hybrid_deep's.
static int hybrid_deep_impl(const char* const who, msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term,
                            const int32_t* q_w, const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas,
                            int n_alphas, uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord,
                            const HybridDeepFilter* flt, uint32_t* out_ord, float* out_score, int32_t* out_n,
                            uint32_t* out_members, uint8_t* out_src, uint32_t* out_sparse_ord, uint32_t* out_sparse_u32,
                            int32_t* out_sparse_n, uint32_t* out_dense_ord, float* out_dense, int32_t* out_dense_n,
                            float* out_range, float* ms) {
    const int n_ms = flt ? 7 : 6;
    if (ms)
        for (int i = 0; i < n_ms; ++i) ms[i] = 0.f;
    // ---- checks, all before any device work: shapes and handles, then ranges, then the device
    if (!ix || !dx || !q_ptr || !row2ord || !alphas || !out_ord || !out_score || !out_n || !out_members || nq < 0 || (nq && !q)) {
        set_error("%s: bad argument", who);
        return MSR_E_INVAL;
    }
    if (int rc0 = dense_precision_check(who, dx, q_is_f32)) return rc0;
    const IndexHeader* h = ix->host.h;
    if (dx->n != h->n_docs) {
        set_error("%s: the dense index holds %llu rows but the sparse index %llu docs", who, (unsigned long long)dx->n,
                  (unsigned long long)h->n_docs);
        return MSR_E_INVAL;
    }
    if (int rc0 = whole_index_check(who, ix)) return rc0;
    for (int i = 0; i < std::min(n_alphas, (int)MSR_SWEEP_MAX_ALPHAS); ++i)
        if (!std::isfinite(alphas[i])) {
            set_error("%s: alphas[%d] is not finite", who, i);
            return MSR_E_INVAL;
        }
    if (flt)
        if (int rc0 = filter_check_shapes(who, flt->set_bits, flt->n_sets, flt->q_set)) return rc0;
    if (depth < 1 || depth > MSR_DEEP_KMAX) {
        set_error("%s: depth must be in [1, MSR_DEEP_KMAX = %d] (got %d)", who, MSR_DEEP_KMAX, depth);
        return MSR_E_RANGE;
    }
    const int k_max = std::min(2 * depth, (int)MSR_DEEP_KMAX);
    if (k < 1 || k > k_max) {
        set_error("%s: k must be in [1, min(2 x depth, MSR_DEEP_KMAX) = %d] (got %d)", who, k_max, k);
        return MSR_E_RANGE;
    }
    if (n_alphas < 1 || n_alphas > MSR_SWEEP_MAX_ALPHAS) {
        set_error("%s: n_alphas must be in [1, %d] (got %d)", who, MSR_SWEEP_MAX_ALPHAS, n_alphas);
        return MSR_E_RANGE;
    }
    if (flt)
        if (int rc0 = filter_check_ranges(who, flt->n_sets, flt->q_set, nq)) return rc0;
    if (h->n_docs > 0x7FFFFFFFull) {
        set_error("%s: %llu docs exceed the 2^31 - 1 columns of a score row", who, (unsigned long long)h->n_docs);
        return MSR_E_RANGE;
    }
    if (int rc0 = device_check(ix)) return rc0;
    if (int rc0 = dense_device_check(who, dx)) return rc0;
    if (ix->dev->device != dx->device) {
        set_error("%s: the sparse and the dense index live on different devices", who);
        return MSR_E_INVAL;
    }
    if (nq == 0) return MSR_OK;
    DeviceIndex* d = ix->dev;
    HIP_TRY(hipSetDevice(d->device));
    const uint32_t n = (uint32_t)h->n_docs;
    if (int rc0 = ensure_ordinal_rows(dx, d->stream, row2ord, h->n_docs)) return rc0;
    // the queries, normalised and uploaded exactly as for a search (refusals included)
    msr_batch* b = nullptr;
    int rc = msr_batch_create(ix, q_ptr, q_term, q_w, nq, 1, flags, &b);
    if (rc != MSR_OK) return rc;
    CallScratch cs(who, d, b);
    // ---- the pass and its scratch (on the dense handle: kept between calls, only ever grown)
    const uint64_t ld_s = (uint64_t)h->n_tiles * h->tile_docs;  // the dump's row: tile t starts at column t * tile_docs
    const uint64_t n_cover = std::min<uint64_t>(dx->n_pad, ((uint64_t)n + 255) / 256 * 256);
    const uint64_t ld_d = std::max<uint64_t>(n_cover, 4);
    // ---- the doc sets, with the call's own upload (bitmap | any | q_set, one block): ONE image over doc ordinals serves
    // both rows, the GEMM runs on the ordinal-ordered rows
    FilterImage fi;
    FilterArgs fa = {};
    bool any_filtered = false;
    for (int i = 0; flt && flt->n_sets > 0 && i < nq && !any_filtered; ++i) any_filtered = !flt->q_set || flt->q_set[i] >= 0;
    if (any_filtered) {
        if (ld_s > 0xFFFFFFFFull || ld_d > ld_s) {  // (a bitmap row covers every vec of both rows: mask_key_rows reads up to ld_d)
            set_error("%s: key rows of %llu columns against doc-set rows of %llu bits", who, (unsigned long long)ld_d,
                      (unsigned long long)ld_s);
            return MSR_E_RANGE;
        }
        fi.build(flt->set_bits, flt->n_sets, flt->q_set, nq, h->n_docs, h->tile_docs, h->n_tiles);
        const size_t o_bits = cs.put(fi.bits), o_any = cs.put(fi.any), o_qs = cs.put(fi.q_set);
        const uint32_t* d_in = cs.upload("doc sets", &rc);
        if (!d_in) return rc;
        fa.bits = d_in + o_bits;
        fa.any = reinterpret_cast<const uint8_t*>(d_in + o_any);
        fa.q_set = reinterpret_cast<const int32_t*>(d_in + o_qs);
        fa.stride = fi.stride;
        fa.n_tiles = h->n_tiles;
    }
    const uint32_t gb = hybrid_gemm_block(dx);
    const uint32_t nq_pad = (uint32_t)(((uint64_t)nq + gb - 1) / gb * gb);
    const uint64_t rb = std::max<uint64_t>(1, kHybridDeepPassBytes / (std::max(ld_s, ld_d) * 4 * gb));
    // (fuse_rows and gather_src take the rows of a pass in grid y: the smallest tile, 4096 docs, bounds a pass at 16 384 rows;
    // the clamp keeps that true whatever tile sizes come)
    const uint32_t qt = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(rb * gb, nq_pad), kMaxGridY / gb * gb);
    const size_t row_bytes = dense_row_bytes(dx), h_row = (size_t)dx->h * (dx->f32 ? 4 : 2);
    const size_t per_d = (size_t)qt * depth, per_k = (size_t)qt * k;
    uint8_t* d_Q = (uint8_t*)dx->take(msr_dense::S_Q, std::max<size_t>((size_t)qt * row_bytes, 16));
    uint32_t* d_S = (uint32_t*)dx->take(msr_dense::S_HD_S, (size_t)qt * ld_s * 4);
    uint32_t* d_D = (uint32_t*)dx->take(msr_dense::S_S, (size_t)qt * ld_d * 4);
    uint32_t* d_F = (uint32_t*)dx->take(msr_dense::S_HD_F, (size_t)qt * ld_s * 4);
    uint32_t* d_sidx = (uint32_t*)dx->take(msr_dense::S_HD_SIDX, per_d * 4);
    uint32_t* d_skey = (uint32_t*)dx->take(msr_dense::S_HD_SKEY, per_d * 4);
    int32_t* d_sn = (int32_t*)dx->take(msr_dense::S_HD_SN, (size_t)qt * 4);
    uint32_t* d_didx = (uint32_t*)dx->take(msr_dense::S_DEEP_IDX, per_d * 4);
    uint32_t* d_dkey = (uint32_t*)dx->take(msr_dense::S_DEEP_KEY, per_d * 4);
    int32_t* d_dn = (int32_t*)dx->take(msr_dense::S_DEEP_N, (size_t)qt * 4);
    uint32_t* d_fidx = (uint32_t*)dx->take(msr_dense::S_HD_FIDX, per_k * 4);
    uint32_t* d_fkey = (uint32_t*)dx->take(msr_dense::S_HD_FKEY, per_k * 4);
    int32_t* d_fn = (int32_t*)dx->take(msr_dense::S_HD_FN, (size_t)qt * 4);
    uint32_t* d_mem = (uint32_t*)dx->take(msr_dense::S_HD_MEM, (size_t)qt * 4);
    float* d_range = (float*)dx->take(msr_dense::S_URANGE, (size_t)qt * 16);
    bool ok = d_Q && d_S && d_D && d_F && d_sidx && d_skey && d_sn && d_didx && d_dkey && d_dn && d_fidx && d_fkey && d_fn &&
              d_mem && d_range;
    uint8_t *d_src = nullptr, *d_fsrc = nullptr;
    if (ok && out_src)
        ok = (d_src = (uint8_t*)dx->take(msr_dense::S_HD_SRC, (size_t)qt * ld_s)) != nullptr &&
             (d_fsrc = (uint8_t*)dx->take(msr_dense::S_HD_FSRC, per_k)) != nullptr;
    int32_t* d_self = nullptr;
    if (ok && self_ord) ok = (d_self = (int32_t*)dx->take(msr_dense::S_SELF, (size_t)nq * 4)) != nullptr;
    if (!ok) {
        set_error("device allocation failed in %s (%u queries per pass x %llu columns, depth %d, k %d)", who, qt,
                  (unsigned long long)std::max(ld_s, ld_d), depth, k);
        return MSR_E_NOMEM;
    }
    if (d_self && !hip_ok(who, hipMemcpyAsync(d_self, self_ord, (size_t)nq * 4, hipMemcpyHostToDevice, d->stream), "upload of self_ord"))
        return MSR_E_HIP;
    // laps of a pass: 0 | scoring | 1 | upload + GEMM | 2 | depth selections | 3, and per alpha 4 + 3a | fuse_rows | 5 + 3a |
    // selection | 6 + 3a (the copies to the host lie between the alphas' laps)
    // (a filtered pass: ... GEMM | 2 | mask_key_rows | lap_mask | depth selections | 3)
    const int lap_mask = 4 + 3 * n_alphas;
    if ((rc = cs.laps(lap_mask + (any_filtered ? 1 : 0), ms != nullptr))) return rc;
    double t[5] = {0, 0, 0, 0, 0}, t_mask = 0;
    uint32_t passes = 0;
    const size_t nqk = (size_t)nq * k;
    for (uint32_t q0 = 0; q0 < (uint32_t)nq; q0 += qt, ++passes) {
        const uint32_t qn = std::min<uint32_t>(qt, (uint32_t)nq - q0);
        const uint32_t qn_pad = (qn + gb - 1) / gb * gb;
        bool pass_filtered = false;
        for (uint32_t i = 0; any_filtered && i < qn && !pass_filtered; ++i) pass_filtered = (int32_t)fi.q_set[q0 + i] >= 0;
        // 1. the sparse dump, exactly as msr_search_deep launches it: row q - q0, column = doc ordinal
        ScoreArgs sa;
        fill_score_args(sa, b, 1);
        sa.part = nullptr;
        sa.q0 = q0;
        sa.qn = qn;
        sa.dump = d_S;
        sa.tpr = h->n_tiles;
        sa.dump_add = 0;
        if ((rc = cs.mark(0))) return rc;
        if ((rc = pass_filtered ? launch_score_dump_filtered(d->stream, h->tile_docs, h->n_tiles, sa, fa)
                                : launch_score_dump(d->stream, h->tile_docs, h->n_tiles, sa)))
            return rc;
        if ((rc = cs.mark(1))) return rc;
        // 2. the hybrid GEMM on the ordinal-ordered rows, writing keys
        if (!upload_query_rows(dx, d_Q, (const uint8_t*)q + (size_t)q0 * h_row, qn, qn_pad, d->stream)) {
            set_error("%s: upload of the query rows failed", who);
            return MSR_E_HIP;
        }
        if ((rc = launch_hybrid_gemm(dx, d_Q, d_D, qn, qn_pad, n_cover, ld_d, d->stream, false))) return rc;
        if ((rc = cs.mark(2))) return rc;
        if (pass_filtered) {  // the dense keys of the non-members become 0 = "no member"
            if ((rc = launch_mask_key_rows(d->stream, d_D, ld_d, qn, q0, fa))) return rc;
            if ((rc = cs.mark(lap_mask))) return rc;
        }
        // 3. both depth lists
        DeepArgs da;
        da.n = n;
        da.rows = qn;
        da.k = (uint32_t)depth;
        da.out_f32 = nullptr;
        da.src = d_S, da.ld = ld_s, da.out_idx = d_sidx, da.out_key = d_skey, da.out_n = d_sn;
        if ((rc = launch_deep_select(d->stream, da))) return rc;
        da.src = d_D, da.ld = ld_d, da.out_idx = d_didx, da.out_key = d_dkey, da.out_n = d_dn;
        if ((rc = launch_deep_select(d->stream, da))) return rc;
        if ((rc = cs.mark(3))) return rc;
        if (!hip_ok(who, hipMemsetAsync(d_mem, 0, (size_t)qn * 4, d->stream), "hipMemsetAsync")) return MSR_E_HIP;
        // 4. per alpha: fuse_rows, the fused top-k, and its copy into the caller's slice
        for (int ai = 0; ai < n_alphas; ++ai) {
            FuseRowsArgs fa;
            fa.S = d_S, fa.D = d_D, fa.ld_s = ld_s, fa.ld_d = ld_d, fa.n = n, fa.depth = (uint32_t)depth;
            fa.self_ord = d_self ? d_self + q0 : nullptr;
            fa.s_idx = d_sidx, fa.s_key = d_skey, fa.s_n = d_sn;
            fa.d_idx = d_didx, fa.d_key = d_dkey, fa.d_n = d_dn;
            fa.w_dense = alphas[ai];
            fa.F = d_F;
            // (members, sources and extremes do not depend on alpha: the first launch writes them)
            fa.src = ai == 0 ? d_src : nullptr;
            fa.members = ai == 0 ? d_mem : nullptr;
            fa.range = ai == 0 ? d_range : nullptr;
            if ((rc = cs.mark(4 + 3 * ai))) return rc;
            hipLaunchKernelGGL(fuse_rows, dim3((uint32_t)((ld_s + kFuseRowsCols - 1) / kFuseRowsCols), qn), dim3(kFuseRowsThreads), 0,
                               d->stream, fa);
            if (!hip_ok(who, hipGetLastError(), "fuse_rows")) return MSR_E_HIP;
            if ((rc = cs.mark(5 + 3 * ai))) return rc;
            da.k = (uint32_t)k;
            da.src = d_F, da.ld = ld_s, da.out_idx = d_fidx, da.out_key = d_fkey, da.out_n = d_fn;
            if ((rc = launch_deep_select(d->stream, da))) return rc;
            if ((rc = cs.mark(6 + 3 * ai))) return rc;
            const size_t o = (size_t)ai * nqk + (size_t)q0 * k, nb = (size_t)qn * k * 4;
            bool c = hipMemcpyAsync(out_ord + o, d_fidx, nb, hipMemcpyDeviceToHost, d->stream) == hipSuccess &&
                     hipMemcpyAsync(out_score + o, d_fkey, nb, hipMemcpyDeviceToHost, d->stream) == hipSuccess &&
                     hipMemcpyAsync(out_n + (size_t)ai * nq + q0, d_fn, (size_t)qn * 4, hipMemcpyDeviceToHost, d->stream) == hipSuccess;
            if (c && out_src) {
                GatherSrcArgs ga;
                ga.src = d_src, ga.ld = ld_s, ga.n = n, ga.idx = d_fidx, ga.k = (uint32_t)k, ga.out = d_fsrc;
                hipLaunchKernelGGL(gather_src, dim3(((uint32_t)k + 255) / 256, qn), dim3(256), 0, d->stream, ga);
                c = hipGetLastError() == hipSuccess &&
                    hipMemcpyAsync(out_src + o, d_fsrc, (size_t)qn * k, hipMemcpyDeviceToHost, d->stream) == hipSuccess;
            }
            if (!c) {
                set_error("%s: download of the fused lists failed: %s", who, hipGetErrorString(hipGetLastError()));
                return MSR_E_HIP;
            }
        }
        // 5. the alpha-independent outputs, then the pass's times
        const size_t od = (size_t)q0 * depth, nbd = (size_t)qn * depth * 4, nbq = (size_t)qn * 4;
        if (!hip_ok(who, hipStreamSynchronize(d->stream), "the kernels of a pass") ||
            !hip_ok(who, hipMemcpy(out_members + q0, d_mem, nbq, hipMemcpyDeviceToHost), "download") ||
            (out_sparse_ord && !hip_ok(who, hipMemcpy(out_sparse_ord + od, d_sidx, nbd, hipMemcpyDeviceToHost), "download")) ||
            (out_sparse_u32 && !hip_ok(who, hipMemcpy(out_sparse_u32 + od, d_skey, nbd, hipMemcpyDeviceToHost), "download")) ||
            (out_sparse_n && !hip_ok(who, hipMemcpy(out_sparse_n + q0, d_sn, nbq, hipMemcpyDeviceToHost), "download")) ||
            (out_dense_ord && !hip_ok(who, hipMemcpy(out_dense_ord + od, d_didx, nbd, hipMemcpyDeviceToHost), "download")) ||
            (out_dense && !hip_ok(who, hipMemcpy(out_dense + od, d_dkey, nbd, hipMemcpyDeviceToHost), "download")) ||
            (out_dense_n && !hip_ok(who, hipMemcpy(out_dense_n + q0, d_dn, nbq, hipMemcpyDeviceToHost), "download")) ||
            (out_range && !hip_ok(who, hipMemcpy(out_range + (size_t)q0 * 4, d_range, (size_t)qn * 16, hipMemcpyDeviceToHost), "download")))
            return MSR_E_HIP;
        for (int i = 0; i < 3; ++i) {
            float x = 0;
            if ((rc = cs.elapsed(i == 2 && pass_filtered ? lap_mask : i, i + 1, &x))) return rc;
            t[i] += x;
        }
        if (pass_filtered) {
            float x = 0;
            if ((rc = cs.elapsed(2, lap_mask, &x))) return rc;
            t_mask += x;
        }
        for (int ai = 0; ai < n_alphas; ++ai) {
            float x = 0, y = 0;
            if ((rc = cs.elapsed(4 + 3 * ai, 5 + 3 * ai, &x)) || (rc = cs.elapsed(5 + 3 * ai, 6 + 3 * ai, &y))) return rc;
            t[3] += x;
            t[4] += y;
        }
    }
    // fused and dense scores travel as order-preserving keys: decoded in place (key 0 = padding = 0.f)
    auto decode = [](float* p, size_t cnt) {
        for (size_t i = 0; i < cnt; ++i) {
            uint32_t key;
            memcpy(&key, p + i, 4);
            const uint32_t bits = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
            if (key) memcpy(p + i, &bits, 4);
        }
    };
    decode(out_score, (size_t)n_alphas * nqk);
    if (out_dense) decode(out_dense, (size_t)nq * depth);
    if (ms) {
        for (int i = 0; i < 5; ++i) ms[i] = (float)t[i];
        ms[5] = (float)passes;
        if (flt) ms[6] = (float)t_mask;
    }
    cs.ok = true;
    return MSR_OK;
}

extern "C" {

int msr_hybrid_deep(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                    const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas, int n_alphas,
                    uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score,
                    int32_t* out_n, uint32_t* out_members, uint8_t* out_src, uint32_t* out_sparse_ord,
                    uint32_t* out_sparse_u32, int32_t* out_sparse_n, uint32_t* out_dense_ord, float* out_dense,
                    int32_t* out_dense_n, float* out_range, float ms[6]) {
    return hybrid_deep_impl("msr_hybrid_deep", ix, dx, q_ptr, q_term, q_w, q, q_is_f32, nq, depth, k, alphas, n_alphas, flags,
                            row2ord, self_ord, nullptr, out_ord, out_score, out_n, out_members, out_src, out_sparse_ord,
                            out_sparse_u32, out_sparse_n, out_dense_ord, out_dense, out_dense_n, out_range, ms);
}

int msr_hybrid_deep_filtered(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                             const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas, int n_alphas,
                             uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord, const uint32_t* set_bits,
                             int n_sets, const int32_t* q_set, uint32_t* out_ord, float* out_score, int32_t* out_n,
                             uint32_t* out_members, uint8_t* out_src, uint32_t* out_sparse_ord, uint32_t* out_sparse_u32,
                             int32_t* out_sparse_n, uint32_t* out_dense_ord, float* out_dense, int32_t* out_dense_n,
                             float* out_range, float ms[7]) {
    const HybridDeepFilter flt = {set_bits, n_sets, q_set};
    return hybrid_deep_impl("msr_hybrid_deep_filtered", ix, dx, q_ptr, q_term, q_w, q, q_is_f32, nq, depth, k, alphas, n_alphas,
                            flags, row2ord, self_ord, &flt, out_ord, out_score, out_n, out_members, out_src, out_sparse_ord,
                            out_sparse_u32, out_sparse_n, out_dense_ord, out_dense, out_dense_n, out_range, ms);
}

}  // extern "C"

// ================================================================================================ encode-side sparsifier
// The step immediately upstream of the index / the query encoder: per row of next-token logits
//     v = log(1 + relu(logit))                       src/model.py:104
//     top-k of v (k = 128 or --sparse_length)        src/encode.py:69-72
//     weight = rint(v * 100) as int                  src/encode.py:75
// One elementwise kernel turns the logits into order-preserving keys of v in the select_tiles layout; selection and
// the tile merge are the kernels of the search path. fp16_math = 1 reproduces a model that runs in fp16 (1 + relu and
// the log are rounded to half before the f32 multiplication by 100), 0 keeps f32 throughout.
namespace msr {

__global__ __launch_bounds__(256) void sparsify_keys(const void* __restrict__ logits, int is_f16, int fp16_math,
                                                     uint32_t* __restrict__ out, uint32_t V, uint64_t ld, uint32_t row0) {
    const uint32_t row = row0 + blockIdx.y;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) {
        float x = is_f16 ? (float)reinterpret_cast<const _Float16*>(logits)[(uint64_t)row * V + i]
                         : reinterpret_cast<const float*>(logits)[(uint64_t)row * V + i];
        float v;
        if (fp16_math) {
            const _Float16 y = (_Float16)((_Float16)1.0f + (_Float16)fmaxf(x, 0.f));  // half add, round to nearest even
            v = (float)(_Float16)logf((float)y);
        } else {
            v = logf(1.0f + fmaxf(x, 0.f));
        }
        out[(uint64_t)row * ld + i] = f32_to_key(v);
    }
}

}  // namespace msr

extern "C" int msr_sparsify(const void* logits, int is_f16, int fp16_math, int rows, uint32_t vocab, int k, int device,
                            uint32_t* out_idx, float* out_val, int32_t* out_weight) {
    if (!logits || rows < 0 || vocab == 0 || !out_idx || !out_val || !out_weight) {
        set_error("msr_sparsify: bad argument");
        return MSR_E_INVAL;
    }
    if (k < 1 || k > MSR_KMAX) {
        set_error("k must be in [1, %d] (got %d)", MSR_KMAX, k);
        return MSR_E_RANGE;
    }
    if ((uint32_t)k > vocab) {  // torch.topk refuses k > vocab too; the selection would pad with id 0xFFFFFFFF
        set_error("k=%d exceeds the vocabulary of %u", k, vocab);
        return MSR_E_RANGE;
    }
    int n_dev = 0;
    if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) {
        set_error("no usable HIP device %d; there is no CPU sparsifier path", device);
        return MSR_E_NODEVICE;
    }
    if (rows == 0) return MSR_OK;
    HIP_TRY(hipSetDevice(device));
    const uint32_t tile = vocab <= 4096 ? 4096 : 8192;
    const uint32_t n_tiles = (vocab + tile - 1) / tile;
    const uint64_t ld = (uint64_t)n_tiles * tile;
    const size_t in_bytes = (size_t)rows * vocab * (is_f16 ? 2 : 4);
    void* d_in = nullptr;
    uint32_t *d_keys = nullptr, *d_ord = nullptr, *d_su = nullptr;
    uint64_t* d_part = nullptr;
    float* d_sf = nullptr;
    int32_t* d_n = nullptr;
    hipStream_t st = nullptr;
    const size_t per = (size_t)rows * k;
    int rc = MSR_OK;
    bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipMalloc(&d_in, in_bytes) == hipSuccess &&
              hipMalloc(&d_keys, (size_t)rows * ld * 4) == hipSuccess && hipMalloc(&d_part, (size_t)n_tiles * per * 8) == hipSuccess &&
              hipMalloc(&d_ord, per * 4) == hipSuccess && hipMalloc(&d_su, per * 4) == hipSuccess &&
              hipMalloc(&d_sf, per * 4) == hipSuccess && hipMalloc(&d_n, (size_t)rows * 4) == hipSuccess &&
              hipMemcpyAsync(d_in, logits, in_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemsetAsync(d_keys, 0, (size_t)rows * ld * 4, st) == hipSuccess;
    if (!ok) {
        set_error("device setup failed in msr_sparsify");
        rc = MSR_E_NOMEM;
    }
    if (rc == MSR_OK) {
        for (uint32_t r0 = 0; r0 < (uint32_t)rows; r0 += kMaxGridY)  // rows in slices of the grid's y limit
            hipLaunchKernelGGL(sparsify_keys,
                               dim3(std::min<uint32_t>((vocab + 255) / 256, 1024), std::min<uint32_t>(kMaxGridY, (uint32_t)rows - r0)),
                               dim3(256), 0, st, d_in, is_f16, fp16_math, d_keys, vocab, ld, r0);
        SelectArgs se;
        se.unsorted = 0;
        se.src = d_keys;
        se.part = d_part;
        se.n_docs = vocab;
        se.n_tiles = n_tiles;
        se.tpr = n_tiles;
        se.rank = 0;
        se.nq = (uint32_t)rows;
        se.q0 = 0;
        se.qn = (uint32_t)rows;
        se.k = (uint32_t)k;
        rc = launch_select(st, tile, se);
    }
    if (rc == MSR_OK) {
        MergeArgs ma;
        ma.lists = d_part;
        ma.list_stride = per;
        ma.n_lists = n_tiles;
        ma.nq = (uint32_t)rows;
        ma.k = (uint32_t)k;
        ma.out_keys = nullptr;
        ma.out_ord = d_ord;
        ma.out_score_u32 = d_su;
        ma.out_score = d_sf;
        ma.out_n = d_n;
        rc = launch_merge(st, ma);
    }
    std::vector<uint32_t> keys(per);
    if (rc == MSR_OK) {
        bool c = hipMemcpyAsync(out_idx, d_ord, per * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipMemcpyAsync(keys.data(), d_su, per * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess;
        if (!c) {
            set_error("sparsifier kernels or download failed: %s", hipGetErrorString(hipGetLastError()));
            rc = MSR_E_HIP;
        }
    }
    if (rc == MSR_OK)
        for (size_t i = 0; i < per; ++i) {
            const uint32_t key = keys[i];
            const uint32_t bits = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
            float v;
            memcpy(&v, &bits, 4);
            if (!key) v = 0.f;
            out_val[i] = v;
            out_weight[i] = (int32_t)nearbyintf(v * 100.0f);  // np.rint(v * 100).astype(int), src/encode.py:75
        }
    void* ptrs[] = {d_in, d_keys, d_part, d_ord, d_su, d_sf, d_n};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (st) (void)hipStreamDestroy(st);
    return rc;
}
