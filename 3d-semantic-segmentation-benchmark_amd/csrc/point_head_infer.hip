// Eval-mode PointNet segmentation head in one pass (reference PointNetEncoder.forward's concatenation,
// PointNet.py:86-90, and PointNetSeg.forward, PointNet.py:140-149, under model.eval()).
//
// The reference builds [g_b expanded over the cloud | pf] (B N x (kg + kp)) and runs conv1 on it.  With
// W1 = [W1g | W1p] in that column order the first layer splits exactly:
//   W1 [g_b ; p] + bias1 = (W1g g_b + bias1) + W1p p
// so the global term is a per-cloud bias.  point_head_bias_kernel forms it once per cloud, BatchNorm
// included:   c[b][j] = s1[j] (sum_k W1[j][k] G[b][k] + bias1[j] - mean1[j]) + beta1[j]
// in fp32 FMAs of a fixed order, and point_head_infer_kernel runs, per tile of 64 rows of ONE cloud,
//   h1 = relu(W1p' p + c[b])   h2 = relu(W2' h1 + b2')   h3 = relu(W3' h2 + b3')   y = W4 h3 + bias4
// and the optional softmax exp(y) / sum exp(y), with eval-mode BatchNorm folded on the device:
//   s = gamma / sqrt(running_var + eps),  W' = s o W,  b' = s o (bias - running_mean) + beta.
// Only the (rows x classes) result reaches HBM: no concatenation, no 512- / 256- / 128-wide activation.
//
// Every layer runs on the bf16 matrix pipe with rows_infer.hip's arithmetic, x w ~= hi_x hi_w + hi_x lo_w
// + lo_x hi_w into one fp32 accumulator; each activation is split into bf16 hi / lo planes once, by the
// epilogue that produces it.  The 512-wide h1 never exists whole: it is produced in chunks of 64 columns
// (its contraction is only kp) and each chunk is consumed at once as two 32-K slabs of h2's accumulators,
// which stay in registers across the eight chunks.
#include <algorithm>

#include "mlp_common.hpp"

namespace pcs {

constexpr int PHI_ROWS = 64;                     // rows of one cloud per block
constexpr int PHI_W1 = 512, PHI_W2 = 256, PHI_W3 = 128;   // the hidden widths this kernel is laid out for
constexpr int PHI_CHUNK = 64;                    // h1 columns per chunk = two K slabs of the second layer
constexpr int PHI_NCHUNK = PHI_W1 / PHI_CHUNK;
constexpr int PHI_MAX_KP = 128, PHI_MAX_CLS = 32;
constexpr int PHI_LD = 2 * 32 + 8;               // one LDS row of a 32-K slab: [32 hi | 32 lo | 8 pad] bf16 = 144 B
constexpr int PHI_IMG = PHI_ROWS * PHI_LD;       // the tile's 64 rows of one slab (bf16 elements), 9216 B
constexpr int PHI_PLANES = 8 * PHI_IMG;          // region A: 8 slab images, 72 KB
constexpr int PHI_H1_SLAB = 4;                   // the chunk's two images sit behind the (up to 4) images of P
constexpr int PHI_STAGE = 256 * PHI_LD;          // one weight stage: 256 (slab, column) rows, 36 KB
constexpr int PHI_NCOEF = PHI_W1 + PHI_W2 + PHI_W3 + PHI_MAX_CLS;   // per-column scale / bias entries
constexpr int PHI_NSTEPS = 3 * PHI_NCHUNK + 4 + 1;
constexpr size_t PHI_LDS = (size_t)(PHI_PLANES + 2 * PHI_STAGE) * sizeof(__bf16) + 2 * PHI_NCOEF * sizeof(float);
constexpr size_t PHI_LDS_LIMIT = 160 * 1024;     // one CU's LDS (gfx950)
static_assert(PHI_LDS <= PHI_LDS_LIMIT, "point head: LDS plan over one CU's LDS");

struct PhiLayer {
    const float *W, *bias, *gamma, *beta, *rm, *rv;
    int ldw, cin, cout;
    float eps;
};

struct PhiArgs {
    PhiLayer L[4];
    const float *P, *G;
    float *cb, *out;                             // cb: the per-cloud biases c (B x 512, the workspace)
    int ldp, ldg, ldo, kg, kp, B, N, tpc, ncls, softmax;   // tpc: tiles per cloud
};

// c[b][j]: one wave per (cloud, column).  Lane l takes k = 4 l + 256 i in ascending i with four FMAs per
// quad, then the 64 partial sums meet in a xor butterfly: a fixed order, the same for every launch.
__global__ __launch_bounds__(256) void point_head_bias_kernel(const PhiArgs A) {
    const PhiLayer& L = A.L[0];
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)A.B * PHI_W1) return;
    const int b = (int)(wid / PHI_W1), j = (int)(wid - (long long)b * PHI_W1);
    const float* wr = L.W + (size_t)j * L.ldw;
    const float* gr = A.G + (size_t)b * A.ldg;
    float acc = 0.f;
    for (int k = 4 * lane; k < A.kg; k += 256) {
        PCS_DCHECK_QUAD(wr + k, L.W, PHI_W1, L.ldw, A.kg, "point head bias W1");
        PCS_DCHECK_QUAD(gr + k, A.G, A.B, A.ldg, A.kg, "point head bias G");
        const float4 w = *reinterpret_cast<const float4*>(wr + k);
        const float4 g = *reinterpret_cast<const float4*>(gr + k);
        acc = __fmaf_rn(w.x, g.x, acc);
        acc = __fmaf_rn(w.y, g.y, acc);
        acc = __fmaf_rn(w.z, g.z, acc);
        acc = __fmaf_rn(w.w, g.w, acc);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) {
        const float s = L.gamma[j] * (1.0f / sqrtf(L.rv[j] + L.eps));
        PCS_DCHECK(wid < (long long)A.B * PHI_W1, "point head bias c cloud %d col %d outside %d x %d", b, j, A.B, PHI_W1);
        A.cb[wid] = s * ((acc + (L.bias ? L.bias[j] : 0.f)) - L.rm[j]) + L.beta[j];
    }
}

// One step of the weight pipeline: ncols = 1 << lgc columns from col0 of `layer`, nsl 32-K slabs from k0
// (ncols nsl <= 256 rows of a stage; row = slab ncols + column).
//   steps 3 c, c < 8:        layer 1, h1 columns 64 c .. + 63, all of kp (nslp <= 4 slabs)
//   steps 3 c + 1, 3 c + 2:  layer 2, all 256 columns, the K slab the chunk's first / second 32 columns are
//   steps 24 .. 27:          layer 3, all 128 columns, two K slabs each
//   step 28:                 the classifier, 32 (zero-padded) class columns, all four K slabs
struct PhiStep {
    int layer, col0, k0, lgc, nsl;
};
__device__ __forceinline__ PhiStep phi_step(int i, int nslp) {
    if (i < 3 * PHI_NCHUNK) {
        const int c = i / 3, j = i - 3 * c;
        if (j == 0) return PhiStep{0, PHI_CHUNK * c, 0, 6, nslp};
        return PhiStep{1, 0, PHI_CHUNK * c + 32 * (j - 1), 8, 1};
    }
    if (i < 3 * PHI_NCHUNK + 4) return PhiStep{2, 0, 64 * (i - 3 * PHI_NCHUNK), 7, 2};
    return PhiStep{3, 0, 0, 5, 4};
}
__device__ __forceinline__ int phi_coef0(int layer) {
    return layer == 0 ? 0 : layer == 1 ? PHI_W1 : layer == 2 ? PHI_W1 + PHI_W2 : PHI_W1 + PHI_W2 + PHI_W3;
}

// relu(v + b) of four consecutive columns -> their hi and lo bf16 (8 B each) at d and d + 32
__device__ __forceinline__ void phi_split4(__bf16* d, const f32x16& acc, int g, const float4 b) {
    const float v0 = fmaxf(acc[4 * g] + b.x, 0.f), v1 = fmaxf(acc[4 * g + 1] + b.y, 0.f);
    const float v2 = fmaxf(acc[4 * g + 2] + b.z, 0.f), v3 = fmaxf(acc[4 * g + 3] + b.w, 0.f);
    const unsigned h0 = bx_pk(v0, v1), h1 = bx_pk(v2, v3);
    // v - float(hi): exact
    const unsigned l0 = bx_pk(v0 - __uint_as_float(h0 << 16), v1 - __uint_as_float(h0 & 0xffff0000u));
    const unsigned l1 = bx_pk(v2 - __uint_as_float(h1 << 16), v3 - __uint_as_float(h1 & 0xffff0000u));
    *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(d + 32) = make_uint2(l0, l1);
}

// the three split terms of one 16-K step, small terms first
#define PHI_MMA3(ACC, WH, WL, XH, XL)                                          \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WH, XL, ACC, 0, 0, 0);       \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WL, XH, ACC, 0, 0, 0);       \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WH, XH, ACC, 0, 0, 0);

// One block = 4 waves = one tile of 64 rows of ONE cloud (tpc = ceil(N / 64) tiles per cloud, the last one
// ragged: row p >= N re-reads row N - 1 and is not written), so c[b] is uniform within the block.
//
// LDS.  Region A, 8 slab images of 64 rows x 144 B (72 KB): first the split planes of P (kp rounded to 32:
// up to 4 images) and, behind them, the two images of the current h1 chunk; after the second layer the 8
// images of h2 over both; after the third layer the 4 images of h3.  Region W: two weight stages of 256
// rows x 144 B (72 KB).  Then 928 column scales s (layers 1-3; 1 for the classifier's classes, 0 beyond)
// and 928 biases (c[b] | b2' | b3' | bias4), 7.25 KB.  151.25 KB in all, one block per CU.
//
// Pipeline.  The 29 steps of phi_step run through one double-buffered stage that never drains: step
// i + 1's weights (each thread owns up to four units of 8 consecutive K values of one column) are loaded
// from L2 before step i's MFMAs and scaled by s, split and written to the other stage after them; one
// barrier per step.  Only the epilogues of the second and third layer, which write planes over images
// other waves were reading in the same step, sit behind a barrier of their own (two per tile).
//
// Fragments.  The weight fragment goes first, so accumulator element 4 g + e of a 32 x 32 tile is
// (column 8 g + 4 h + e, row l32): a lane holds four consecutive columns of one row per g, which an
// epilogue turns into one 8-B hi and one 8-B lo write, and the classifier's lane pair (h = 0, 1) holds
// all 32 classes of a row, so the softmax is 16 in-lane terms and one __shfl_xor(.., 32).
//   layer 1: wave (wm, wn) owns rows 32 wm .. x chunk columns 32 wn ..           1 tile,  16 accumulators
//   layer 2: wave w owns all 64 rows x columns 64 w .. + 63                       2 x 2,  64, live over the chunks
//   layer 3: wave w owns all 64 rows x columns 32 w .. + 31                       2 x 1,  32
//   classifier: waves 0 and 1 own rows 32 w .. x the 32 class columns            1 tile,  16
__global__ __launch_bounds__(256) void point_head_infer_kernel(const PhiArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char phi_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.x / A.tpc, tile = blockIdx.x - b * A.tpc;
    const int N = A.N, r0 = tile * PHI_ROWS, nv = min(PHI_ROWS, N - r0);
    const int kp = A.kp, nslp = (kp + 31) >> 5;
    __bf16* Ab = reinterpret_cast<__bf16*>(phi_lds);
    __bf16* Wd = Ab + PHI_PLANES;
    float* sc = reinterpret_cast<float*>(Wd + 2 * PHI_STAGE);
    float* bs = sc + PHI_NCOEF;

    // s (the arithmetic of bn_eval_coef_kernel, engine.hip) and the biases
    for (int e = tid; e < PHI_NCOEF; e += 256) {
        float s, bb;
        if (e < PHI_W1) {
            s = A.L[0].gamma[e] * (1.0f / sqrtf(A.L[0].rv[e] + A.L[0].eps));
            PCS_DCHECK(b < A.B, "point head c cloud %d outside %d", b, A.B);
            bb = A.cb[(size_t)b * PHI_W1 + e];
        } else if (e < PHI_W1 + PHI_W2 + PHI_W3) {
            const PhiLayer& L = A.L[e < PHI_W1 + PHI_W2 ? 1 : 2];
            const int n = e - (e < PHI_W1 + PHI_W2 ? PHI_W1 : PHI_W1 + PHI_W2);
            PCS_DCHECK(n < L.cout, "point head coefficient %d outside %d", n, L.cout);
            s = L.gamma[n] * (1.0f / sqrtf(L.rv[n] + L.eps));
            bb = s * ((L.bias ? L.bias[n] : 0.f) - L.rm[n]) + L.beta[n];
        } else {
            const int n = e - (PHI_W1 + PHI_W2 + PHI_W3);
            s = n < A.ncls ? 1.f : 0.f;
            bb = n < A.ncls && A.L[3].bias ? A.L[3].bias[n] : 0.f;
        }
        sc[e] = s;
        bs[e] = bb;
    }
    // the tile's rows of P, split once: consecutive threads take consecutive 8-K units of a row; channels at
    // or beyond kp are written as zeros whatever the pad columns hold
    {
        const int upr = 4 * nslp;
        for (int u = tid; u < PHI_ROWS * upr; u += 256) {
            const int r = u / upr, q = u - r * upr, k = 8 * q;
            const float* pp = A.P + ((size_t)b * N + min(r0 + r, N - 1)) * A.ldp + k;
            float4 xa = make_float4(0.f, 0.f, 0.f, 0.f), xb = xa;
            if (k < kp) {
                PCS_DCHECK_QUAD(pp, A.P, (long long)A.B * N, A.ldp, kp, "point head P");
                xa = *reinterpret_cast<const float4*>(pp);
            }
            if (k + 4 < kp) {
                PCS_DCHECK_QUAD(pp + 4, A.P, (long long)A.B * N, A.ldp, kp, "point head P");
                xb = *reinterpret_cast<const float4*>(pp + 4);
            }
            uint4 hi, lo;
            bx_split8(xa, xb, hi, lo);
            __bf16* d = Ab + (q >> 2) * PHI_IMG + r * PHI_LD + 8 * (q & 3);
            *reinterpret_cast<uint4*>(d) = hi;
            *reinterpret_cast<uint4*>(d + 32) = lo;
        }
    }
    __syncthreads();               // load_w reads sc

    float4 wa[4], wb[4];
    float sv[4];
    int nun = 0;                   // units of the step in wa / wb
    auto load_w = [&](int i) {
        const PhiStep S = phi_step(i, nslp);
        const PhiLayer& L = A.L[S.layer];
        const int koff = S.layer == 0 ? A.kg : 0;          // W1's point columns follow its kg global ones
        const int kend = S.layer == 0 ? kp : L.cin;
        const int cf = phi_coef0(S.layer);
        nun = (4 << S.lgc) * S.nsl;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int unit = tid + 256 * u;
            const int n = S.col0 + ((unit >> 2) & ((1 << S.lgc) - 1));
            const int k = S.k0 + 32 * (unit >> (S.lgc + 2)) + 8 * (unit & 3);
            wa[u] = wb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            sv[u] = 0.f;
            if (unit < nun && n < L.cout) {
                const float* wp = L.W + (size_t)n * L.ldw + koff + k;
                if (k < kend) {
                    PCS_DCHECK_QUAD(wp, L.W, L.cout, L.ldw, koff + kend, "point head W");
                    wa[u] = *reinterpret_cast<const float4*>(wp);
                }
                if (k + 4 < kend) {
                    PCS_DCHECK_QUAD(wp + 4, L.W, L.cout, L.ldw, koff + kend, "point head W");
                    wb[u] = *reinterpret_cast<const float4*>(wp + 4);
                }
                sv[u] = sc[cf + n];
            }
        }
    };
    auto store_w = [&](int stage) {
        __bf16* Ws = Wd + stage * PHI_STAGE;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int unit = tid + 256 * u;
            if (unit >= nun) break;
            const float s = sv[u];
            uint4 hi, lo;
            bx_split8(make_float4(s * wa[u].x, s * wa[u].y, s * wa[u].z, s * wa[u].w),
                      make_float4(s * wb[u].x, s * wb[u].y, s * wb[u].z, s * wb[u].w), hi, lo);
            __bf16* d = Ws + (unit >> 2) * PHI_LD + 8 * (unit & 3);        // row = slab ncols + column
            *reinterpret_cast<uint4*>(d) = hi;
            *reinterpret_cast<uint4*>(d + 32) = lo;
        }
    };

    load_w(0);
    store_w(0);
    __syncthreads();

    const int fo = l32 * PHI_LD + 8 * h;                   // a lane's fragment offset inside a 32-row image
    const int wm = wave & 1, wn = wave >> 1;
    __bf16* H1 = Ab + PHI_H1_SLAB * PHI_IMG;
    f32x16 acc2[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc2[i][j] = f32x16{};

    int step = 0;
    for (int c = 0; c < PHI_NCHUNK; ++c) {
        // ---- layer 1, chunk c: relu(W1p' p + c[b]) -> the chunk's two images
        load_w(step + 1);
        {
            f32x16 a1 = f32x16{};
            const __bf16* Xs = Ab + 32 * wm * PHI_LD + fo;
            const __bf16* Ws = Wd + (step & 1) * PHI_STAGE + 32 * wn * PHI_LD + fo;
            for (int s = 0; s < nslp; ++s)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 xh = *reinterpret_cast<const bf16x8*>(Xs + s * PHI_IMG + 16 * ks);
                    const bf16x8 xl = *reinterpret_cast<const bf16x8*>(Xs + s * PHI_IMG + 16 * ks + 32);
                    const bf16x8 wh = *reinterpret_cast<const bf16x8*>(Ws + s * PHI_CHUNK * PHI_LD + 16 * ks);
                    const bf16x8 wl = *reinterpret_cast<const bf16x8*>(Ws + s * PHI_CHUNK * PHI_LD + 16 * ks + 32);
                    PHI_MMA3(a1, wh, wl, xh, xl)
                }
            // the chunk's readers (the previous chunk's layer-2 steps) are at least one barrier behind
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bv = *reinterpret_cast<const float4*>(bs + PHI_CHUNK * c + 32 * wn + 8 * g + 4 * h);
                phi_split4(H1 + wn * PHI_IMG + (32 * wm + l32) * PHI_LD + 8 * g + 4 * h, a1, g, bv);
            }
        }
        store_w((step + 1) & 1);
        __syncthreads();
        ++step;
        // ---- layer 2: the chunk's two images are K slabs 2 c and 2 c + 1
        for (int t = 0; t < 2; ++t) {
            load_w(step + 1);                               // step + 1 <= 24 < PHI_NSTEPS
            const __bf16* Xs = H1 + t * PHI_IMG + fo;
            const __bf16* Ws = Wd + (step & 1) * PHI_STAGE + 64 * wave * PHI_LD + fo;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 xh[2], xl[2], wh[2], wl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    xh[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * PHI_LD + 16 * ks);
                    xl[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * PHI_LD + 16 * ks + 32);
                    wh[i] = *reinterpret_cast<const bf16x8*>(Ws + 32 * i * PHI_LD + 16 * ks);
                    wl[i] = *reinterpret_cast<const bf16x8*>(Ws + 32 * i * PHI_LD + 16 * ks + 32);
                }
                // the three terms outermost: four independent accumulators between two MFMAs on the same one
#define PHI_MMA(WF, XF)                                                                                      \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) acc2[i][j] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(WF[j], XF[i], acc2[i][j], 0, 0, 0);
                PHI_MMA(wh, xl) PHI_MMA(wl, xh) PHI_MMA(wh, xh)
#undef PHI_MMA
            }
            store_w((step + 1) & 1);
            __syncthreads();
            ++step;
        }
    }
    // ---- layer 2's epilogue: h2's 8 images over P and the last chunk (every reader is behind the barrier)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bv = *reinterpret_cast<const float4*>(bs + PHI_W1 + 64 * wave + 32 * j + 8 * g + 4 * h);
                phi_split4(Ab + (2 * wave + j) * PHI_IMG + (32 * i + l32) * PHI_LD + 8 * g + 4 * h, acc2[i][j], g, bv);
            }
    __syncthreads();

    // ---- layer 3: four steps of two K slabs
    f32x16 acc3[2] = {f32x16{}, f32x16{}};
    for (int q = 0; q < 4; ++q) {
        load_w(step + 1);
        const __bf16* Xs = Ab + 2 * q * PHI_IMG + fo;
        const __bf16* Ws = Wd + (step & 1) * PHI_STAGE + 32 * wave * PHI_LD + fo;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 wh = *reinterpret_cast<const bf16x8*>(Ws + sl * PHI_W3 * PHI_LD + 16 * ks);
                const bf16x8 wl = *reinterpret_cast<const bf16x8*>(Ws + sl * PHI_W3 * PHI_LD + 16 * ks + 32);
                bf16x8 xh[2], xl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    xh[i] = *reinterpret_cast<const bf16x8*>(Xs + sl * PHI_IMG + 32 * i * PHI_LD + 16 * ks);
                    xl[i] = *reinterpret_cast<const bf16x8*>(Xs + sl * PHI_IMG + 32 * i * PHI_LD + 16 * ks + 32);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) acc3[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xl[i], acc3[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i) acc3[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xh[i], acc3[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 2; ++i) acc3[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh[i], acc3[i], 0, 0, 0);
            }
        store_w((step + 1) & 1);
        __syncthreads();
        ++step;
    }
    // h3's 4 images over h2 (every reader of h2 is behind the barrier)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bv = *reinterpret_cast<const float4*>(bs + PHI_W1 + PHI_W2 + 32 * wave + 8 * g + 4 * h);
            phi_split4(Ab + wave * PHI_IMG + (32 * i + l32) * PHI_LD + 8 * g + 4 * h, acc3[i], g, bv);
        }
    __syncthreads();

    // ---- classifier (+ softmax): waves 0 and 1, 32 rows each; class 8 g + 4 h + e of row 32 wave + l32
    if (wave >= 2) return;
    f32x16 y = f32x16{};
    {
        const __bf16* Xs = Ab + 32 * wave * PHI_LD + fo;
        const __bf16* Ws = Wd + (step & 1) * PHI_STAGE + fo;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 xh = *reinterpret_cast<const bf16x8*>(Xs + s * PHI_IMG + 16 * ks);
                const bf16x8 xl = *reinterpret_cast<const bf16x8*>(Xs + s * PHI_IMG + 16 * ks + 32);
                const bf16x8 wh = *reinterpret_cast<const bf16x8*>(Ws + s * PHI_MAX_CLS * PHI_LD + 16 * ks);
                const bf16x8 wl = *reinterpret_cast<const bf16x8*>(Ws + s * PHI_MAX_CLS * PHI_LD + 16 * ks + 32);
                PHI_MMA3(y, wh, wl, xh, xl)
            }
    }
    const float* b4 = bs + PHI_W1 + PHI_W2 + PHI_W3;
    const int ncls = A.ncls;
    float m = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cls = 8 * (r >> 2) + 4 * h + (r & 3);
        y[r] += b4[cls];
        if (cls < ncls) m = fmaxf(m, y[r]);
    }
    if (A.softmax) {
        // exp(y - max) / sum: equal to the reference's exp(y) / sum exp(y) wherever that is finite
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cls = 8 * (r >> 2) + 4 * h + (r & 3);
            y[r] = cls < ncls ? expf(y[r] - m) : 0.f;
            sum += y[r];
        }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] *= inv;
    }
    const int row = 32 * wave + l32;
    if (row < nv) {
        float* op = A.out + ((size_t)b * N + r0 + row) * A.ldo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cls = 8 * (r >> 2) + 4 * h + (r & 3);
            if (cls < ncls) {
                PCS_DCHECK(r0 + row < N && b < A.B, "point head out cloud %d row %d col %d outside %d x %d x %d", b, r0 + row,
                           cls, A.B, N, ncls);
                op[cls] = y[r];
            }
        }
    }
}
#undef PHI_MMA3

// Every limit of the head lives here (before any GPU work); fills the layers and sizes.
static int phi_check(const char* who, int B, int N, int kg, const pcs_mlp_layer* layers, int nl, PhiArgs& a) {
    static const int widths[3] = {PHI_W1, PHI_W2, PHI_W3};
    PCS_CHECK_ARG(layers, "%s: null pointer", who);
    PCS_CHECK_ARG(nl == 4, "%s: %d layers (4: three hidden layers and the classifier)", who, nl);
    PCS_CHECK_ARG(B >= 1 && N >= 1 && (long long)B * N < (1ll << 31), "%s: bad sizes B=%d N=%d", who, B, N);
    PCS_CHECK_ARG(kg >= 4 && kg % 4 == 0 && kg < (1 << 24), "%s: kg %d (%% 4 == 0, >= 4)", who, kg);
    const long long kp = layers[0].cin - kg;
    PCS_CHECK_ARG(kp >= 4 && kp % 4 == 0 && kp <= PHI_MAX_KP, "%s: kp %lld = layer 0 cin %lld - kg %d (%% 4 == 0, 4 .. %d)",
                  who, kp, (long long)layers[0].cin, kg, PHI_MAX_KP);
    long long cin = kg + kp;
    for (int l = 0; l < nl; ++l) {
        const pcs_mlp_layer& R = layers[l];
        const bool last = l == nl - 1;
        PCS_CHECK_ARG(R.W, "%s: layer %d null pointer", who, l);
        PCS_CHECK_ARG(R.use_batch == 0, "%s: layer %d BatchNorm is in training mode", who, l);
        if (last) {
            PCS_CHECK_ARG(!R.gamma && !R.beta && !R.run_mean && !R.run_var,
                          "%s: the last layer carries a BatchNorm (the classifier is bias only)", who);
            PCS_CHECK_ARG(R.act == ACT_NONE, "%s: the last layer's activation %lld (none)", who, (long long)R.act);
            PCS_CHECK_ARG(R.cout >= 1 && R.cout <= PHI_MAX_CLS, "%s: classes %lld (1 .. %d)", who, (long long)R.cout,
                          PHI_MAX_CLS);
        } else {
            PCS_CHECK_ARG(R.gamma && R.beta && R.run_mean && R.run_var, "%s: layer %d null pointer", who, l);
            PCS_CHECK_ARG(R.act == ACT_RELU, "%s: layer %d activation %lld (ReLU)", who, l, (long long)R.act);
            PCS_CHECK_ARG(R.cout == widths[l], "%s: layer %d width %lld (the hidden widths are %d, %d, %d)", who, l,
                          (long long)R.cout, PHI_W1, PHI_W2, PHI_W3);
        }
        PCS_CHECK_ARG(R.cin == cin && R.ldw >= cin && R.ldw < (1ll << 24), "%s: layer %d cin %lld ldw %lld (expected cin %lld)",
                      who, l, (long long)R.cin, (long long)R.ldw, cin);
        PCS_CHECK_ARG(R.ldw % 4 == 0 && (reinterpret_cast<uintptr_t>(R.W) & 15) == 0,
                      "%s: layer %d W must be 16-B aligned with ldw %% 4 == 0 (ldw %lld)", who, l, (long long)R.ldw);
        a.L[l] = PhiLayer{R.W, R.bias, R.gamma, R.beta, R.run_mean, R.run_var, (int)R.ldw, (int)R.cin, (int)R.cout, (float)R.eps};
        cin = R.cout;
    }
    PCS_CHECK_ARG(PHI_LDS <= PHI_LDS_LIMIT, "%s: the stack needs %zu B of LDS (limit %zu)", who, PHI_LDS, PHI_LDS_LIMIT);
    a.kg = kg, a.kp = (int)kp, a.B = B, a.N = N, a.ncls = (int)layers[nl - 1].cout;
    a.tpc = (N + PHI_ROWS - 1) / PHI_ROWS;
    PCS_CHECK_ARG((long long)B * a.tpc < (1ll << 31), "%s: too many tiles", who);
    return 0;
}

}  // namespace pcs

using namespace pcs;

// Workspace bytes of pcs_point_head_infer (the per-cloud biases c, B x 512 floats); non-zero (with a
// message) when the head is not covered -- the coverage test of the bindings.
PCS_API int pcs_point_head_infer_workspace(int B, int N, int kg, const pcs_mlp_layer* layers, int nl, size_t* bytes) {
    PCS_CHECK_ARG(bytes, "pcs_point_head_infer_workspace: null pointer");
    PhiArgs a{};
    if (int rc = phi_check("pcs_point_head_infer_workspace", B, N, kg, layers, nl, a)) return rc;
    *bytes = (size_t)B * PHI_W1 * sizeof(float);
    return 0;
}

// Eval-mode PointNet segmentation head.  P (B*N rows of kp channels, row stride ldp; cloud b = rows b N ..
// b N + N - 1), G (B x kg, row stride ldg); layers: 4 pcs_mlp_layer records (W .. slope), layers[0].cin =
// kg + kp with W1's columns [0, kg) on G and [kg, kg + kp) on P; out (B*N x classes, row stride ldo).
// Reference: PointNet.py:86-90, 140-149 under eval().
PCS_API int pcs_point_head_infer(const float* P, int ldp, const float* G, int ldg, int kg, int B, int N,
                                 const pcs_mlp_layer* layers, int nl, int softmax, float* out, int ldo, void* ws,
                                 size_t ws_bytes, void* stream) {
    PCS_CHECK_ARG(P && G && out && ws, "pcs_point_head_infer: null pointer");
    PhiArgs a{};
    if (int rc = phi_check("pcs_point_head_infer", B, N, kg, layers, nl, a)) return rc;
    PCS_CHECK_ARG(ldp % 4 == 0 && ldp >= a.kp && (reinterpret_cast<uintptr_t>(P) & 15) == 0,
                  "pcs_point_head_infer: ldp %d (%% 4 == 0, >= kp %d; P 16-B aligned)", ldp, a.kp);
    PCS_CHECK_ARG(ldg % 4 == 0 && ldg >= kg && (reinterpret_cast<uintptr_t>(G) & 15) == 0,
                  "pcs_point_head_infer: ldg %d (%% 4 == 0, >= kg %d; G 16-B aligned)", ldg, kg);
    PCS_CHECK_ARG(ldo >= a.ncls && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "pcs_point_head_infer: ldo %d (>= classes %d)",
                  ldo, a.ncls);
    const size_t need = (size_t)B * PHI_W1 * sizeof(float);
    PCS_CHECK_ARG(ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                  "pcs_point_head_infer: workspace %zu B (needs %zu)", ws_bytes, need);
    a.P = P, a.G = G, a.out = out, a.cb = static_cast<float*>(ws);
    a.ldp = ldp, a.ldg = ldg, a.ldo = ldo, a.softmax = softmax != 0;
    hipStream_t st = as_stream(stream);
    // 151 KB of dynamic LDS: above the 64 KB default cap
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&point_head_infer_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)PHI_LDS);
    (void)attr;
    const double w1g = (double)kg * PHI_W1;
    {
        ProbeScope pr(st, 2.0 * B * w1g, 4.0 * (w1g + (double)B * kg + (double)B * PHI_W1), "pcs::point_head_bias_kernel");
        hipLaunchKernelGGL(point_head_bias_kernel, dim3((unsigned)(((long long)B * PHI_W1 + 3) / 4)), dim3(256), 0, st, a);
    }
    if (int rc = launch_status("pcs_point_head_infer")) return rc;
    const double wts = (double)a.kp * PHI_W1 + (double)PHI_W1 * PHI_W2 + (double)PHI_W2 * PHI_W3 + (double)PHI_W3 * a.ncls;
    {
        // compulsory bytes: P, c and the weights read once, out written
        ProbeScope pr(st, 2.0 * B * N * wts, 4.0 * ((double)B * N * (a.kp + a.ncls) + wts + (double)B * PHI_W1),
                      "pcs::point_head_infer_kernel");
        hipLaunchKernelGGL(point_head_infer_kernel, dim3(B * a.tpc), dim3(256), PHI_LDS, st, a);
    }
    return launch_status("pcs_point_head_infer");
}
