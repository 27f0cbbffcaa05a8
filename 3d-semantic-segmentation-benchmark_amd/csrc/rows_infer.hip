// Eval-mode conv + BatchNorm + activation on rows for the wide, un-pooled layers of an inference
// forward (DGCNN's head conv5-7, the FeaturePropagation stacks, the UnitPointNet of an InvResMLP, the
// PointNeXt stem; reference UnitPointNet, common.py:153-178, and dgcnn.py:188-210 under model.eval()):
//
//   Y = act( s o (X W^T) + t ),   s = gamma / sqrt(running_var + eps),  t = s o (bias - running_mean) + beta
//   (no BatchNorm: s = 1, t = bias)
//
// on the bf16 matrix pipe with fp32 storage on both sides.  Each fp32 operand is split on its way into
// LDS, x = hi + lo with hi = bf16(x) (round to nearest even) and lo = bf16(x - hi) (the difference is
// exact), and the product keeps the three leading terms
//   x w ~= hi_x hi_w + hi_x lo_w + lo_x hi_w        (lo_x lo_w ~ 2^-18 |x w| is dropped)
// as three v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator: about 16 significand bits per operand.
// The error against fp64 is set by the split (~4e-6 norm-relative, independent of cin); fp32 accumulation
// adds ~2e-7, so a second accumulator for the two small terms would cost 64 registers and an epilogue add
// for nothing measurable.  s and t are applied to the accumulator, not folded into W before the split:
// gamma == 0 gives act(beta) exactly.
#include "mlp_common.hpp"

namespace pcs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int RI_BM = 128;               // rows of X per block tile (64 per wave)
constexpr int RI_BN = 128;               // columns of Y per block tile (64 per wave)
constexpr int RI_BK = 32;                // K slab: two MFMA K steps
// One LDS row of a tile = [32 hi | 32 lo | 8 pad] bf16 = 144 B: the two planes of a row side by side,
// the same bytes the fp32 slab had, + 16 B.  36 dwords = 4 mod 8, so the 16 lanes of a ds_read_b128
// phase (16 consecutive rows, one 16-B unit each) fall on distinct banks.
constexpr int RI_LD = 2 * RI_BK + 8;
constexpr int RI_TILE = 128 * RI_LD;     // bf16 elements of one operand tile (X or W)
constexpr int RI_STAGE = 2 * RI_TILE;    // X tile, W tile
constexpr size_t RI_LDS = 2 * RI_STAGE * sizeof(__bf16) + 2 * RI_BN * sizeof(float);   // 2 stages + s, t: 73 KB

struct RiArgs {
    const float *X, *W, *bias, *gamma, *beta, *rm, *rv;
    float* Y;
    int ldx, ldw, ldy, M, cin, cout, tm, tn;
    float eps, slope;                    // slope: the activation's effective slope (eff_slope)
};

// two floats -> two bf16 (RNE) in one dword: v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned ri_pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// 8 consecutive K values -> their hi and lo units (8 bf16 = 16 B each)
__device__ __forceinline__ void ri_split8(const float4 a, const float4 b, uint4& hi, uint4& lo) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned h[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        h[p] = ri_pk(x[2 * p], x[2 * p + 1]);
        // x - float(hi): exact (hi is x rounded to 8 significand bits)
        l[p] = ri_pk(x[2 * p] - __uint_as_float(h[p] << 16), x[2 * p + 1] - __uint_as_float(h[p] & 0xffff0000u));
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}

// One block = 4 waves = one 128 x 128 tile of Y; wave (wm, wn) owns the 64 x 64 quarter at rows 64 wm,
// columns 64 wn as 2 x 2 MFMA tiles (64 accumulator registers).
//
// Staging.  A K slab of 32 is 128 rows x 4 units of 8 consecutive K values per operand; thread t owns
// units t and t + 256 of X and of W (4 lanes cover a row's 128 B).  LDS-DMA cannot convert, so a unit
// travels global -> registers (two float4) -> ri_split8 -> two ds_write_b128 (hi, lo).  The slabs are
// pipelined through a double-buffered stage: slab s + 1's global loads are issued before slab s's MFMAs
// and split + written into the other stage after them, one barrier per slab.  K is zero-extended to
// the slab (cin % 4 == 0: a quad is loaded or zero); rows at or beyond M re-read row M - 1 (never
// stored), weight rows at or beyond cout are zero.  W is split by every block while staging: splitting
// it once per launch into bf16 planes in a workspace measured slower.
//
// MFMA.  The A operand is the weight fragment and B the X fragment (lane l32 = the tile's row, lane
// half h = K values 8 h .. + 7 of the step: one ds_read_b128 each), so accumulator element 4 g + e of a
// tile is (column 8 g + 4 h + e, row l32): four consecutive columns of one row per lane, and the
// epilogue's s / t, activation and stores are float4.  Per K step: 8 fragment reads, 12 MFMAs, the three
// terms outermost so that four independent accumulators separate two MFMAs on the same one.
//
// Tile order.  Blocks b, b + 8, .. run on one XCD; there the column tiles of one row tile are
// consecutive, so an X tile comes from HBM once and from that XCD's L2 for the other column tiles.
__global__ __launch_bounds__(256, 2) void rows_infer_kernel(const RiArgs A) {
    extern __shared__ __attribute__((aligned(16))) __bf16 ri_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const int rt = (li / A.tn) * 8 + xcd, ct = li % A.tn;
    if (rt >= A.tm) return;
    const int row0 = rt * RI_BM, col0 = ct * RI_BN;
    const int M = A.M, cin = A.cin, cout = A.cout;
    float* sc = reinterpret_cast<float*>(ri_lds + 2 * RI_STAGE);      // s, then t, of this block's columns
    float* tc = sc + RI_BN;

    // BN's scale and shift (s: the arithmetic of bn_eval_coef_kernel, engine.hip); read after the first barrier
    if (tid < RI_BN) {
        const int n = col0 + tid;
        float s = 0.f, t = 0.f;
        if (n < cout) {
            const float b = A.bias ? A.bias[n] : 0.f;
            if (A.gamma) {
                s = A.gamma[n] * (1.0f / sqrtf(A.rv[n] + A.eps));
                t = s * (b - A.rm[n]) + A.beta[n];
            } else {
                s = 1.f, t = b;
            }
        }
        sc[tid] = s;
        tc[tid] = t;
    }

    // this thread's two units of either operand tile: row ur[u], K offset uk[u] within the slab
    int ur[2], uk[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = tid + 256 * u;
        ur[u] = q >> 2;
        uk[u] = 8 * (q & 3);
    }
    float4 xa[2], xb[2], wa[2], wb[2];
    auto load_slab = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = k0 + uk[u];
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float* xp = A.X + (size_t)min(row0 + ur[u], M - 1) * A.ldx + k;
            xa[u] = xb[u] = z;
            if (k < cin) {
                PCS_DCHECK_QUAD(xp, A.X, M, A.ldx, cin, "rows infer X");
                xa[u] = *reinterpret_cast<const float4*>(xp);
            }
            if (k + 4 < cin) {
                PCS_DCHECK_QUAD(xp + 4, A.X, M, A.ldx, cin, "rows infer X");
                xb[u] = *reinterpret_cast<const float4*>(xp + 4);
            }
            const int n = col0 + ur[u];
            const float* wp = A.W + (size_t)min(n, cout - 1) * A.ldw + k;
            wa[u] = wb[u] = z;
            if (n < cout && k < cin) {
                PCS_DCHECK_QUAD(wp, A.W, cout, A.ldw, cin, "rows infer W");
                wa[u] = *reinterpret_cast<const float4*>(wp);
            }
            if (n < cout && k + 4 < cin) {
                PCS_DCHECK_QUAD(wp + 4, A.W, cout, A.ldw, cin, "rows infer W");
                wb[u] = *reinterpret_cast<const float4*>(wp + 4);
            }
        }
    };
    auto store_slab = [&](int stage) {
        __bf16* Xs = ri_lds + stage * RI_STAGE;
        __bf16* Ws = Xs + RI_TILE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int o = ur[u] * RI_LD + uk[u];
            uint4 hi, lo;
            ri_split8(xa[u], xb[u], hi, lo);
            *reinterpret_cast<uint4*>(Xs + o) = hi;
            *reinterpret_cast<uint4*>(Xs + o + RI_BK) = lo;
            ri_split8(wa[u], wb[u], hi, lo);
            *reinterpret_cast<uint4*>(Ws + o) = hi;
            *reinterpret_cast<uint4*>(Ws + o + RI_BK) = lo;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};

    const int nslab = (cin + RI_BK - 1) / RI_BK;
    load_slab(0);
    store_slab(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
        const bool more = s + 1 < nslab;
        if (more) load_slab((s + 1) * RI_BK);          // in flight across this slab's MFMAs
        const __bf16* Xs = ri_lds + (s & 1) * RI_STAGE + (64 * wm + l32) * RI_LD + 8 * h;
        const __bf16* Ws = ri_lds + (s & 1) * RI_STAGE + RI_TILE + (64 * wn + l32) * RI_LD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < RI_BK / 16; ++ks) {
            bf16x8 xh[2], xl[2], wh[2], wl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                xh[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * RI_LD + 16 * ks);
                xl[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * RI_LD + 16 * ks + RI_BK);
                wh[i] = *reinterpret_cast<const bf16x8*>(Ws + 32 * i * RI_LD + 16 * ks);
                wl[i] = *reinterpret_cast<const bf16x8*>(Ws + 32 * i * RI_LD + 16 * ks + RI_BK);
            }
#define RI_MMA(WF, XF)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(WF[j], XF[i], acc[i][j], 0, 0, 0);
            RI_MMA(wl, xh) RI_MMA(wh, xl) RI_MMA(wh, xh)
#undef RI_MMA
        }
        if (more) store_slab((s + 1) & 1);
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = row0 + 64 * wm + 32 * i + l32;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int nl = 64 * wn + 32 * j + 8 * g + 4 * h, n = col0 + nl;
                if (n >= cout) continue;                 // cout % 4 == 0: a quad is inside or outside
                const float4 sv = *reinterpret_cast<const float4*>(sc + nl);
                const float4 tv = *reinterpret_cast<const float4*>(tc + nl);
                float* yp = A.Y + (size_t)m * A.ldy + n;
                PCS_DCHECK_QUAD(yp, A.Y, M, A.ldy, cout, "rows infer Y");
                *reinterpret_cast<float4*>(yp) = make_float4(act_f(acc[i][j][4 * g] * sv.x + tv.x, 0, A.slope),
                                                             act_f(acc[i][j][4 * g + 1] * sv.y + tv.y, 0, A.slope),
                                                             act_f(acc[i][j][4 * g + 2] * sv.z + tv.z, 0, A.slope),
                                                             act_f(acc[i][j][4 * g + 3] * sv.w + tv.w, 0, A.slope));
            }
    }
}

}  // namespace pcs

using namespace pcs;

// Eval-mode layer on rows: Y (M x cout, row stride ldy) = act(s o (X W^T) + t) with X (M x cin, row
// stride ldx) and the fields W .. slope of one pcs_mlp_layer record (W, bias, gamma, beta and the running
// statistics are only read).  gamma, beta, run_mean, run_var all null: a bare linear layer with bias.
PCS_API int pcs_rows_infer(const float* X, int ldx, long long M, const pcs_mlp_layer* layer, float* Y, int ldy,
                           void* stream) {
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    PCS_CHECK_ARG(X && layer && Y && layer->W, "pcs_rows_infer: null pointer");
    const pcs_mlp_layer& L = *layer;
    const bool bn = L.gamma || L.beta || L.run_mean || L.run_var;
    PCS_CHECK_ARG(!bn || (L.gamma && L.beta && L.run_mean && L.run_var),
                  "pcs_rows_infer: BatchNorm needs gamma, beta and both running statistics (or none of them)");
    PCS_CHECK_ARG(!bn || L.use_batch == 0, "pcs_rows_infer: BatchNorm is in training mode");
    PCS_CHECK_ARG(M >= 1 && M < (1ll << 31) && L.cin >= 4 && L.cin % 4 == 0 && L.cin < (1 << 24) && L.cout >= 4 &&
                      L.cout % 4 == 0 && L.cout < (1 << 24),
                  "pcs_rows_infer: bad sizes M=%lld cin=%lld cout=%lld (cin, cout >= 4 and %% 4 == 0)", M,
                  (long long)L.cin, (long long)L.cout);
    PCS_CHECK_ARG(ldx % 4 == 0 && ldx >= L.cin && L.ldw % 4 == 0 && L.ldw >= L.cin && L.ldw < (1ll << 31) &&
                      ldy % 4 == 0 && ldy >= L.cout,
                  "pcs_rows_infer: strides ldx=%d ldw=%lld ldy=%d (%% 4 == 0, >= cin=%lld / cin / cout=%lld)", ldx,
                  (long long)L.ldw, ldy, (long long)L.cin, (long long)L.cout);
    PCS_CHECK_ARG(al16(X) && al16(L.W) && al16(Y), "pcs_rows_infer: X, W, Y must be 16-B aligned");
    PCS_CHECK_ARG(L.act >= ACT_RELU && L.act <= ACT_NONE && (L.act != ACT_LRELU || L.slope >= 0.0),
                  "pcs_rows_infer: activation %lld slope %g (ReLU, LeakyReLU(slope >= 0) or none)", (long long)L.act, L.slope);
    RiArgs a{};
    a.X = X, a.W = L.W, a.bias = L.bias, a.gamma = L.gamma, a.beta = L.beta, a.rm = L.run_mean, a.rv = L.run_var;
    a.Y = Y, a.ldx = ldx, a.ldw = (int)L.ldw, a.ldy = ldy, a.M = (int)M, a.cin = (int)L.cin, a.cout = (int)L.cout;
    a.tm = (int)((M + RI_BM - 1) / RI_BM), a.tn = (a.cout + RI_BN - 1) / RI_BN;
    a.eps = (float)L.eps, a.slope = eff_slope((int)L.act, (float)L.slope);
    const long long blocks = 8ll * ((a.tm + 7) / 8) * a.tn;
    PCS_CHECK_ARG(blocks < (1ll << 31), "pcs_rows_infer: too many tiles");
    hipStream_t st = as_stream(stream);
    const double flops = 2.0 * (double)M * a.cin * a.cout;
    // compulsory bytes: X and W read once, Y written
    const double bytes = 4.0 * ((double)M * a.cin + (double)a.cout * a.cin + (double)M * a.cout);
    // 73 KB of dynamic LDS: above the 64 KB default cap, two blocks per CU
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&rows_infer_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)RI_LDS);
    (void)attr;
    ProbeScope pr(st, flops, bytes, "pcs::rows_infer_kernel");
    hipLaunchKernelGGL(rows_infer_kernel, dim3((int)blocks), dim3(256), RI_LDS, st, a);
    return launch_status("pcs_rows_infer");
}
