// Wide-layer weight gradient on plain operands on the bf16 matrix pipe, for training (opt-in:
// PCS_WGRAD_BF16X3 in a layer's bwd_fuse field): part[split][n][k] = sum over the split's rows m of
// X[m][n] * Y[m][k], X = the layer's materialised dZ (M x N, row stride ldx), Y = its plain input
// (M x K, row stride ldy); wgrad_reduce_kernel then adds the splits into dW (N x K) in split order.
// The split-bf16 counterpart of wgrad_kernel<128, 128, 0, 0, 1> (mlp.hip) / wgrad_nt_kernel
// (gemm_big.hip) for DGCNN's conv5..conv7 (models/dgcnn/dgcnn.py:188-207) over B*N = 131072 rows.
//
// Arithmetic: gemm_big_bf16x3.hip's.  Storage is fp32 on both sides; x = hi + lo with hi = bf16(x)
// (RNE), lo = bf16(x - hi), and a product keeps hi hi + hi lo + lo hi as three
// v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator (~4e-6 norm-relative against fp64).
//
// Design (CDNA4).  The contraction axis is the ROW m, strided in memory, while an MFMA lane needs 8
// consecutive m of one channel in a single ds_read_b128: the split transposes on its way into LDS.
//  * LDS image = gemm_nt_bf16x3's with "row" = channel and "K" = sample row: per channel
//    [32 hi | 32 lo | 8 pad] bf16 = 144 B = 36 dwords = 4 mod 8, the X tile's 256 channels, then the
//    Y tile's 128; 2 stages x 384 x 144 B = 110592 B (108 KB), one workgroup per CU.  The fragment
//    addressing, the reads' bank argument and the 12-MFMA K step are that kernel's;
//  * 256 (dZ channels n) x 128 (input channels k) output tile per 512-thread workgroup, 8 waves as
//    4 x 2, each a 64 x 64 block as 2 x 2 MFMA tiles (64 accumulator registers);
//  * staging unit = 8 consecutive rows x 4 channels: eight float4 loads -> transposed in registers
//    (pure renaming) -> per channel one bx_split8 -> one ds_write_b128 for hi, one for lo.  A 32-row
//    slab has (64 + 32) channel quads x 4 row groups = 384 units: waves 0..3 take X's 256, waves 4, 5
//    Y's 128, one unit per lane; waves 6 and 7 stage nothing (they wait at the barrier; two of the
//    four SIMDs carry two staging waves, two carry one -- ~500 VALU cycles per unit against 1536
//    MFMA cycles per SIMD and slab);
//  * lane -> unit map: lane = ql | g << 2 | qh << 4, channel quad 16 wave + 4 qh + ql, row group g.
//    Global: one load instruction reads 4 rows x 256 contiguous bytes (16 quads).  LDS: the write of
//    channel j of a unit lands at dword (4 quad + j) * 36 + 4 g (+ 16 for lo) = 16 (quad mod 4) + 4 g
//    + const (mod 64): the 16 lanes of a ds_write_b128 phase (ql x g) cover the 16 four-bank groups
//    once -- 0 conflicts in all 8 writes of a unit.  (Lanes on consecutive quads with one row group,
//    the coalescing-first map, sit 576 B = 16 banks apart: 4 lanes per bank group, 4-way conflicts);
//  * slab s + 1's global loads are issued before slab s's MFMAs, split and written into the other
//    stage after them: one barrier per slab;
//  * rows are split over workgroups (wgrad_bf16x3_plan: ~512 workgroups, splits a multiple of 32 rows);
//    every element of part[split] is written by exactly one workgroup and the splits are added in
//    split order in fp64: identical calls give bitwise-identical dW;
//  * XCD-aware tile order (wgrad_nt_kernel's bijective remap, tile fastest): the tiles of one row
//    split read the same X / Y rows on one L2;
//  * edges: M arbitrary -- a row at or beyond the split's end would reach EVERY output, so its source
//    address is clamped to the split's last row and its value zeroed (a select, not a product) before
//    the split: hi = lo = 0.  Channel quads at or beyond N / K re-read the last valid quad; their
//    products are not stored.  N % 4 == 0, K % 4 == 0, ldx / ldy multiples of 4 >= N / K, 16-B aligned.
#include "mlp_common.hpp"

namespace pcs {

constexpr int WB_BN = 256;               // dZ channels per block tile (the MFMA A operand)
constexpr int WB_BK = 128;               // input channels per block tile (the B operand)
constexpr int WB_BR = 32;                // sample rows per slab: two MFMA K steps
constexpr int WB_LD = 2 * WB_BR + 8;     // bf16 per LDS channel row: [32 hi | 32 lo | 8 pad]
constexpr int WB_STAGE = (WB_BN + WB_BK) * WB_LD;
constexpr int WB_STAGERS = (WB_BN + WB_BK) / 4 * (WB_BR / 8) / 64;   // waves that stage: one unit per lane
static_assert(2 * WB_STAGE * sizeof(__bf16) == 110592 && WB_STAGERS == 6 && WB_BN / 64 == 4, "wgrad_bf16x3 tile");

__device__ __forceinline__ float wb_get(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

__global__ __launch_bounds__(512, 1) void wgrad_bf16x3_kernel(const float* __restrict__ X, int ldx,
                                                              const float* __restrict__ Y, int ldy, int M, int N, int K,
                                                              int rows_per_split, int tiles_k, int tiles,
                                                              float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * WB_STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                 // 4 x 2 waves of 64 x 64
    const int h = lane >> 5, l32 = lane & 31;

    // XCD remap, then tile-fastest: the tiles of one row split (same X / Y rows) share an L2
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
    const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
    const int sp = t / tiles, ti = t - sp * tiles;
    const int n0 = (ti / tiles_k) * WB_BN, k0 = (ti % tiles_k) * WB_BK;
    const int rb = sp * rows_per_split, re = min(M, rb + rows_per_split);   // the split's rows: rb < re
    const int ns = (re - rb + WB_BR - 1) / WB_BR;

    // this lane's staging unit: channel quad uq of the slab's 96 (X's 64, then Y's 32), row group g
    const bool stager = wave < WB_STAGERS, isx = wave < WB_BN / 64;
    const int g = (lane >> 2) & 3;
    const int uq = stager ? 16 * wave + 4 * (lane >> 4) + (lane & 3) : WB_BN / 4;   // (idle waves: unused)
    const int ld = isx ? ldx : ldy;
    const float* src = isx ? X + min(n0 + 4 * uq, N - 4) : Y + min(k0 + 4 * (uq - WB_BN / 4), K - 4);
    float4 gv[8];
    auto load_slab = [&](int s) {
        const int r0 = rb + s * WB_BR + 8 * g;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* p = src + (size_t)min(r0 + i, re - 1) * ld;
            if (isx) PCS_DCHECK_QUAD(p, X, M, ldx, N, "wgrad_bf16x3 X");
            else PCS_DCHECK_QUAD(p, Y, M, ldy, K, "wgrad_bf16x3 Y");
            gv[i] = *reinterpret_cast<const float4*>(p);
        }
    };
    auto store_slab = [&](int stage, int s) {
        const int nv = re - (rb + s * WB_BR + 8 * g);        // rows of this group inside the split
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i >= nv) gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        __bf16* d = lds + stage * WB_STAGE + 4 * uq * WB_LD + 8 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 hi, lo;
            bx_split8(make_float4(wb_get(gv[0], j), wb_get(gv[1], j), wb_get(gv[2], j), wb_get(gv[3], j)),
                      make_float4(wb_get(gv[4], j), wb_get(gv[5], j), wb_get(gv[6], j), wb_get(gv[7], j)), hi, lo);
            *reinterpret_cast<uint4*>(d + j * WB_LD) = hi;
            *reinterpret_cast<uint4*>(d + j * WB_LD + WB_BR) = lo;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

    if (stager) {
        load_slab(0);
        store_slab(0, 0);
    }
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        const bool more = stager && s + 1 < ns;
        if (more) load_slab(s + 1);                    // in flight across this slab's MFMAs
        const __bf16* Xs = lds + (s & 1) * WB_STAGE + (64 * wm + l32) * WB_LD + 8 * h;
        const __bf16* Ys = lds + (s & 1) * WB_STAGE + (WB_BN + 64 * wn + l32) * WB_LD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < WB_BR / 16; ++ks) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * WB_LD + 16 * ks);
                al[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * WB_LD + 16 * ks + WB_BR);
                bh[i] = *reinterpret_cast<const bf16x8*>(Ys + 32 * i * WB_LD + 16 * ks);
                bl[i] = *reinterpret_cast<const bf16x8*>(Ys + 32 * i * WB_LD + 16 * ks + WB_BR);
            }
#define WB_MMA(AF, BF)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[i], BF[j], acc[i][j], 0, 0, 0);
            WB_MMA(ah, bl) WB_MMA(al, bh) WB_MMA(ah, bh)
#undef WB_MMA
        }
        if (more) store_slab((s + 1) & 1, s + 1);
        __syncthreads();
    }

    // lane (h, l32) holds input channel (column) l32 of each tile, dZ channels (r & 3) + 8 (r >> 2) + 4 h
    float* __restrict__ tp = part + (size_t)sp * N * K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + 64 * wn + 32 * j + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + 64 * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < N && k < K) {
                    PCS_DCHECK(sp >= 0 && n >= 0 && k >= 0, "wgrad_bf16x3 part: split %d n %d k %d outside %d x %d", sp,
                               n, k, N, K);
                    tp[(size_t)n * K + k] = acc[i][j][r];
                }
            }
        }
}

// ~512 workgroups (two per CU's worth of the chip, as wgrad_nt_plan): row splits a multiple of 32 rows
static void wgrad_bf16x3_plan(int N, int K, int M, int* tiles_k, int* tiles, int* splits, int* rows) {
    *tiles_k = (K + WB_BK - 1) / WB_BK;
    *tiles = ((N + WB_BN - 1) / WB_BN) * *tiles_k;
    const int sp = (512 + *tiles - 1) / *tiles;
    int r = (M + sp - 1) / sp;
    r = ((r + WB_BR - 1) / WB_BR) * WB_BR;
    *rows = r;
    *splits = (M + r - 1) / r;
}

bool wgrad_bf16x3_args_ok(const float* X, int ldx, const float* Y, int ldy, int M, int N, int K) {
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return X && Y && M >= 1 && N >= 4 && K >= 4 && N % 4 == 0 && K % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 &&
           ldx >= N && ldy >= K && al16(X) && al16(Y);
}

// The engine's predicate: the wide regime.  Measured in-step on DGCNN's head.
bool wgrad_bf16x3_ok(const float* X, int ldx, const float* Y, int ldy, int M, int N, int K) {
    return M >= 65536 && wgrad_bf16x3_args_ok(X, ldx, Y, ldy, M, N, K);
}

size_t wgrad_bf16x3_ws_bytes(int N, int K, int M) {
    if (M <= 0) return 0;
    int tk, tiles, sp, rows;
    wgrad_bf16x3_plan(N, K, M, &tk, &tiles, &sp, &rows);
    return (size_t)sp * N * K * sizeof(float) + 256;
}

int wgrad_bf16x3(const float* X, int ldx, const float* Y, int ldy, int M, int N, int K, float* dW, void* ws,
                 size_t ws_bytes, hipStream_t st) {
    const size_t need = wgrad_bf16x3_ws_bytes(N, K, M);
    PCS_CHECK_ARG(ws && ws_bytes >= need, "pcs_wgrad_bf16x3: workspace too small (%zu < %zu)", ws_bytes, need);
    int tk, tiles, sp, rows;
    wgrad_bf16x3_plan(N, K, M, &tk, &tiles, &sp, &rows);
    PCS_CHECK_ARG((long long)sp * tiles < (1ll << 31), "pcs_wgrad_bf16x3: too many tiles");
    float* part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
    {
        // compulsory bytes: X and Y read once, the partial tiles written
        ProbeScope pr(st, 2.0 * M * N * K, 4.0 * ((double)M * (N + K) + (double)sp * N * K),
                      "pcs::wgrad_bf16x3_kernel");
        hipLaunchKernelGGL(wgrad_bf16x3_kernel, dim3((unsigned)(sp * tiles)), dim3(512), 0, st, X, ldx, Y, ldy, M, N, K,
                           rows, tk, tiles, part);
    }
    wgrad_reduce_launch(part, sp, (long long)N * K, dW, nullptr, N, nullptr, st);
    return launch_status("pcs_wgrad_bf16x3");
}

}  // namespace pcs

using namespace pcs;

PCS_API int pcs_wgrad_bf16x3_workspace(int N, int K, int M, size_t* bytes) {
    PCS_CHECK_ARG(bytes && N >= 1 && K >= 1 && M >= 0, "pcs_wgrad_bf16x3_workspace: bad arguments");
    *bytes = wgrad_bf16x3_ws_bytes(N, K, M);
    return 0;
}

// dW (N x K, contiguous) += X[M x N]^T (ldx) . Y[M x K] (ldy) on the bf16 matrix pipe with split fp32 operands
PCS_API int pcs_wgrad_bf16x3(const float* X, int ldx, const float* Y, int ldy, int M, int N, int K, float* dW,
                             void* workspace, size_t ws_bytes, void* stream) {
    PCS_CHECK_ARG(dW && wgrad_bf16x3_args_ok(X, ldx, Y, ldy, M, N, K),
                  "pcs_wgrad_bf16x3: needs M >= 1, N and K >= 4 and %% 4 == 0, ldx / ldy multiples of 4 >= N / K, 16-B "
                  "aligned X and Y, dW (M=%d N=%d K=%d ldx=%d ldy=%d)", M, N, K, ldx, ldy);
    return wgrad_bf16x3(X, ldx, Y, ldy, M, N, K, dW, workspace, ws_bytes, as_stream(stream));
}
