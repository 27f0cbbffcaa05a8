// Wide-layer GEMM on plain operands on the bf16 matrix pipe, for training (opt-in: PCS_GEMM_BF16X3 in a
// layer's bwd_fuse field): C[M x N] = A[M x R] . B[N x R]^T (+ bias), the split-bf16 counterpart of
// gemm_nt (gemm_big.hip) with its BN-statistics epilogue.  The engine runs a wide layer's forward on it
// (A = the layer input, B = W) and its data gradient (A = the materialised dZ, B = W^T): DGCNN's
// conv5..conv7 (models/dgcnn/dgcnn.py:188-207) over B*N = 131072 rows.
//
// Arithmetic (that of rows_infer.hip).  Storage is fp32 on both sides.  Each operand is split on its
// way into LDS, x = hi + lo with hi = bf16(x) (round to nearest even) and lo = bf16(x - float(hi)) (the
// difference is exact), and the product keeps
//   a b ~= hi_a hi_b + hi_a lo_b + lo_a hi_b        (lo_a lo_b ~ 2^-18 |a b| is dropped)
// as three v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator: ~4e-6 norm-relative against fp64.
//
// Design (CDNA4):
//  * 256 x 128 output tile per 512-thread workgroup, 8 waves as 4 x 2, each wave a 64 x 64 block as
//    2 x 2 MFMA tiles (64 accumulator registers).  Against rows_infer's 128 x 128 tile a B (weight)
//    slab is fetched, split and written to LDS once per 256 rows instead of once per 128;
//  * K in 32-deep slabs, two LDS stages.  LDS-DMA cannot convert, so a slab is register-staged: units
//    of 8 consecutive K values travel global (two float4) -> split -> two ds_write_b128 (hi, lo).
//    Thread t owns units t and t + 512 of A's 1024 and unit t of B's 512 (4 lanes cover a row's 128 B).
//    Slab s + 1's global loads are issued before slab s's MFMAs and split + written into the other
//    stage after them: one barrier per slab;
//  * one LDS row of a tile = [32 hi | 32 lo | 8 pad] bf16 = 144 B = 36 dwords = 4 mod 8, so the 16
//    lanes of a ds_read_b128 phase (16 consecutive rows, one 16-B unit each) fall on distinct banks.
//    2 stages x (256 + 128) rows x 144 B = 110592 B (108 KB): one workgroup per CU;
//  * MFMA: A operand = the A-row fragment, B operand = the B-row fragment (lane l32 = the tile's row,
//    lane half h = K values 8h .. 8h + 7 of the 16-deep step: one ds_read_b128 each), so accumulator
//    element r of lane (h, l32) is (row (r & 3) + 8 (r >> 2) + 4 h, column l32) -- gemm_nt's layout,
//    so a lane's 32 x 2 elements of one column are summed in registers for the statistics.  Per K
//    step: 8 fragment reads, 12 MFMAs, the three terms outermost so that four independent
//    accumulators separate two MFMAs on the same one;
//  * XCD-aware tile order (gemm_nt's bijective remap of the 1-D grid): each XCD walks a contiguous run
//    of tiles, so the column tiles of one 256-row A strip run on one L2 at the same time;
//  * B is split by every block while staging (no per-launch bf16 planes in a workspace: nothing to
//    allocate, nothing extra to capture in a HIP graph);
//  * edges: R % 32 == 0, so a slab is always full.  A rows at or beyond M re-read row M - 1 and B
//    rows at or beyond N row N - 1 (always in bounds); their products are neither stored nor counted;
//  * epilogue: bias, store, and (STATS) per-column fp64 (sum, sum of squares) of the tile's valid rows
//    into the BN partial layout [2][N][row tiles] that bn_finalize reads (256-row tiles, as gemm_nt).
#include "mlp_common.hpp"

namespace pcs {

constexpr int BX_BM = 256;               // rows of A per block tile (= gemm_nt's row tile: the stats layout)
constexpr int BX_BN = 128;               // columns of C per block tile
constexpr int BX_BK = 32;                // K slab: two MFMA K steps
constexpr int BX_LD = 2 * BX_BK + 8;     // bf16 per LDS row: [32 hi | 32 lo | 8 pad]
constexpr int BX_STAGE = (BX_BM + BX_BN) * BX_LD;   // bf16 per stage: the A tile, then the B tile
static_assert(2 * BX_STAGE * sizeof(__bf16) == 110592, "bf16x3 LDS budget");

// the operand split (bx_pk / bx_split8) and the bf16 vector types: mlp_common.hpp

template <bool STATS>
__global__ __launch_bounds__(512, 1) void gemm_nt_bf16x3_kernel(const float* __restrict__ A, int lda,
                                                                const float* __restrict__ B, int ldb, int M, int N,
                                                                int R, const float* __restrict__ bias,
                                                                float* __restrict__ C, int ldc,
                                                                double* __restrict__ stats, int ntn, int mtiles) {
    // one array: the two stages, reused by the epilogue for the statistics reduction
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BX_STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                 // 4 x 2 waves of 64 x 64
    const int h = lane >> 5, l32 = lane & 31;

    // bijective XCD remap: blocks bid, bid + 8, ... share an XCD; give them consecutive tiles
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
    const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
    const int mt = t / ntn, nt = t - mt * ntn;
    const int m0 = mt * BX_BM, n0 = nt * BX_BN;

    // this thread's units: rows (tid >> 2) and (tid >> 2) + 128 of the A tile, row tid >> 2 of the B
    // tile, K offset 8 (tid & 3) within the slab; source rows clamped in range
    const int ur = tid >> 2, uk = 8 * (tid & 3);
    const float* ap0 = A + (size_t)min(m0 + ur, M - 1) * lda + uk;
    const float* ap1 = A + (size_t)min(m0 + ur + 128, M - 1) * lda + uk;
    const float* bp = B + (size_t)min(n0 + ur, N - 1) * ldb + uk;
    float4 ga[4], gb[2];
    auto load_slab = [&](int k0) {
        PCS_DCHECK_QUAD(ap0 + k0, A, M, lda, R, "gemm_nt_bf16x3 A");
        PCS_DCHECK_QUAD(ap0 + k0 + 4, A, M, lda, R, "gemm_nt_bf16x3 A");
        PCS_DCHECK_QUAD(ap1 + k0, A, M, lda, R, "gemm_nt_bf16x3 A");
        PCS_DCHECK_QUAD(ap1 + k0 + 4, A, M, lda, R, "gemm_nt_bf16x3 A");
        PCS_DCHECK_QUAD(bp + k0, B, N, ldb, R, "gemm_nt_bf16x3 B");
        PCS_DCHECK_QUAD(bp + k0 + 4, B, N, ldb, R, "gemm_nt_bf16x3 B");
        ga[0] = *reinterpret_cast<const float4*>(ap0 + k0);
        ga[1] = *reinterpret_cast<const float4*>(ap0 + k0 + 4);
        ga[2] = *reinterpret_cast<const float4*>(ap1 + k0);
        ga[3] = *reinterpret_cast<const float4*>(ap1 + k0 + 4);
        gb[0] = *reinterpret_cast<const float4*>(bp + k0);
        gb[1] = *reinterpret_cast<const float4*>(bp + k0 + 4);
    };
    auto store_slab = [&](int stage) {
        __bf16* As = lds + stage * BX_STAGE + ur * BX_LD + uk;
        __bf16* Bs = lds + stage * BX_STAGE + (BX_BM + ur) * BX_LD + uk;
        uint4 hi, lo;
        bx_split8(ga[0], ga[1], hi, lo);
        *reinterpret_cast<uint4*>(As) = hi;
        *reinterpret_cast<uint4*>(As + BX_BK) = lo;
        bx_split8(ga[2], ga[3], hi, lo);
        *reinterpret_cast<uint4*>(As + 128 * BX_LD) = hi;
        *reinterpret_cast<uint4*>(As + 128 * BX_LD + BX_BK) = lo;
        bx_split8(gb[0], gb[1], hi, lo);
        *reinterpret_cast<uint4*>(Bs) = hi;
        *reinterpret_cast<uint4*>(Bs + BX_BK) = lo;
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

    const int ns = R / BX_BK;
    load_slab(0);
    store_slab(0);
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        const bool more = s + 1 < ns;
        if (more) load_slab((s + 1) * BX_BK);          // in flight across this slab's MFMAs
        const __bf16* As = lds + (s & 1) * BX_STAGE + (64 * wm + l32) * BX_LD + 8 * h;
        const __bf16* Bs = lds + (s & 1) * BX_STAGE + (BX_BM + 64 * wn + l32) * BX_LD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < BX_BK / 16; ++ks) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(As + 32 * i * BX_LD + 16 * ks);
                al[i] = *reinterpret_cast<const bf16x8*>(As + 32 * i * BX_LD + 16 * ks + BX_BK);
                bh[i] = *reinterpret_cast<const bf16x8*>(Bs + 32 * i * BX_LD + 16 * ks);
                bl[i] = *reinterpret_cast<const bf16x8*>(Bs + 32 * i * BX_LD + 16 * ks + BX_BK);
            }
#define BX_MMA(AF, BF)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[i], BF[j], acc[i][j], 0, 0, 0);
            BX_MMA(ah, bl) BX_MMA(al, bh) BX_MMA(ah, bh)
#undef BX_MMA
        }
        if (more) store_slab((s + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: lane (h, l32) holds column l32 of each tile, rows (r & 3) + 8 (r >> 2) + 4 h
    double s1[2], s2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + 64 * wn + 32 * j + l32;
        const bool cok = col < N;
        const float bv = (bias && cok) ? bias[col] : 0.f;
        s1[j] = 0.0;
        s2[j] = 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rb = m0 + 64 * wm + 32 * i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = acc[i][j][r] + bv;
                const bool ok = cok && row < M;
                if (ok) {
                    PCS_DCHECK(row >= 0 && col >= 0 && col < ldc, "gemm_nt_bf16x3 C: row %d col %d outside %d x %d (ld %d)",
                               row, col, M, N, ldc);
                    C[(size_t)row * ldc + col] = v;
                }
                if (STATS) {
                    const double d = ok ? (double)v : 0.0;
                    s1[j] += d;
                    s2[j] += d * d;
                }
            }
        }
    }
    if (STATS) {
        // the last slab's barrier is behind every wave's fragment reads: the stages are free
        double* red = reinterpret_cast<double*>(lds);        // [2][4 row waves][BX_BN]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double a = s1[j] + __shfl_xor(s1[j], 32);
            const double b = s2[j] + __shfl_xor(s2[j], 32);
            const int lc = 64 * wn + 32 * j + l32;
            if (lane < 32) {
                red[wm * BX_BN + lc] = a;
                red[(4 + wm) * BX_BN + lc] = b;
            }
        }
        __syncthreads();
        if (tid < BX_BN && n0 + tid < N) {
            const int col = n0 + tid;
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { a += red[w * BX_BN + tid]; b += red[(4 + w) * BX_BN + tid]; }
            stats[(size_t)col * mtiles + mt] = a;
            stats[((size_t)N + col) * mtiles + mt] = b;
        }
    }
}

bool gemm_nt_bf16x3_args_ok(const float* A, int lda, const float* B, int ldb, int M, int N, int R, const float* C,
                            int ldc) {
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return A && B && C && M >= 1 && N >= 4 && N % 4 == 0 && R >= BX_BK && R % BX_BK == 0 && lda % 4 == 0 && lda >= R &&
           ldb % 4 == 0 && ldb >= R && ldc % 4 == 0 && ldc >= N && al16(A) && al16(B) && al16(C);
}

int gemm_nt_bf16x3(const float* A, int lda, const float* B, int ldb, int M, int N, int R, const float* bias, float* C,
                   int ldc, double* stats, hipStream_t st) {
    const int mtiles = gemm_nt_row_tiles(M);
    const int ntn = (N + BX_BN - 1) / BX_BN;
    const long long tiles = (long long)mtiles * ntn;
    PCS_CHECK_ARG(tiles < (1ll << 31), "gemm_nt_bf16x3: too many tiles");
    const dim3 grid((unsigned)tiles);
    // compulsory bytes: A and B read once, C written
    ProbeScope pr(st, 2.0 * M * N * R, 4.0 * ((double)M * R + (double)N * R + (double)M * N),
                  "pcs::gemm_nt_bf16x3_kernel<%s>", stats ? "true" : "false");
    if (stats)
        hipLaunchKernelGGL(gemm_nt_bf16x3_kernel<true>, grid, dim3(512), 0, st, A, lda, B, ldb, M, N, R, bias, C, ldc,
                           stats, ntn, mtiles);
    else
        hipLaunchKernelGGL(gemm_nt_bf16x3_kernel<false>, grid, dim3(512), 0, st, A, lda, B, ldb, M, N, R, bias, C, ldc,
                           stats, ntn, mtiles);
    return launch_status("gemm_nt_bf16x3");
}

}  // namespace pcs

using namespace pcs;

// C[M x N] (ldc) = A[M x R] (lda) . B[N x R]^T (ldb) (+ bias) on the bf16 matrix pipe with split fp32
// operands; stats (nullable): [2][N][pcs_gemm_nt_row_tiles(M)] fp64 (sum, sum of squares) partials of C.
PCS_API int pcs_gemm_nt_bf16x3(const float* A, int lda, const float* B, int ldb, int M, int N, int R,
                               const float* bias, float* C, int ldc, double* stats, void* stream) {
    PCS_CHECK_ARG(gemm_nt_bf16x3_args_ok(A, lda, B, ldb, M, N, R, C, ldc),
                  "pcs_gemm_nt_bf16x3: needs M >= 1, N >= 4 and %% 4 == 0, R >= 32 and %% 32 == 0, lda/ldb/ldc multiples "
                  "of 4 >= R / R / N, 16-B aligned A, B, C (M=%d N=%d R=%d lda=%d ldb=%d ldc=%d)", M, N, R, lda, ldb, ldc);
    return gemm_nt_bf16x3(A, lda, B, ldb, M, N, R, bias, C, ldc, stats, as_stream(stream));
}
