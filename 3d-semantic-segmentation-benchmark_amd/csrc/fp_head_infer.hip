// Eval-mode full-resolution tail of the PointNet++ family in one pass: the last FeaturePropagation
// (reference common.py:115-122, 217-243: 3-NN inverse-distance interpolation, skip concatenation, shared
// MLP) and the model's classifier (PointNetpp.py:46-47) under model.eval():
//   x  = [f1[row] | interp(f2[b])[row]]                                 D1 + 128 channels, never in HBM
//   h1 = relu(W1' x + b1')  ..  h_nl = relu(W_nl' h_(nl-1) + b_nl')      128 wide each
//   y  = W_c h_nl + bias_c                                               1 .. 32 classes
// with eval-mode BatchNorm folded on the device: s = gamma / sqrt(running_var + eps), W' = s o W,
// b' = s o (bias - running_mean) + beta.  The interpolated quad is interp_cat_q_kernel's (gather.hip)
// per-element fp32 arithmetic, so layer 1 sees the numbers the layered path feeds it.  Every layer runs on
// the bf16 matrix pipe with rows_infer.hip's arithmetic, x w ~= hi_x lo_w + lo_x hi_w + hi_x hi_w into one
// fp32 accumulator.  Only the (rows x classes) logits reach HBM (and, on request, the ReLU decisions).
#include <algorithm>

#include "mlp_common.hpp"

namespace pcs {

constexpr int FPH_ROWS = 128;                    // rows per block (any clouds: the cloud index is per row)
constexpr int FPH_W = 128;                       // the hidden width and D2, the coarse features' width
constexpr int FPH_MAX_D1 = 32, FPH_MAX_CLS = 32, FPH_MAX_NL = 4;
constexpr int FPH_NSLAB = (FPH_MAX_D1 + FPH_W + 31) / 32;   // 32-K slabs of layer 1's input: up to 5
constexpr int FPH_LD = 2 * 32 + 8;               // one LDS row of a 32-K slab: [32 hi | 32 lo | 8 pad] bf16 = 144 B
constexpr int FPH_IMG = FPH_ROWS * FPH_LD;       // the tile's 128 rows of one slab (bf16 elements), 18 KB
constexpr int FPH_STAGE = FPH_W * FPH_LD;        // one weight stage: 128 (slab, column) rows of one slab, 18 KB
constexpr int FPH_NCOEF = FPH_MAX_NL * FPH_W + FPH_MAX_CLS;
constexpr int FPH_INFO = 8;                      // per row: 3 coarse rows, 3 weights, their sum, pad
// LDS plan: activations in place (5 images, 90 KB), two weight stages (36 KB), scales and biases (4.25 KB),
// the rows' interpolation records (4 KB): 134.25 KB, one block per CU
constexpr size_t FPH_LDS = (size_t)(FPH_NSLAB * FPH_IMG + 2 * FPH_STAGE) * sizeof(__bf16) +
                           (2 * FPH_NCOEF + FPH_ROWS * FPH_INFO) * sizeof(float);
constexpr size_t FPH_LDS_LIMIT = 160 * 1024;     // one CU's LDS (gfx950)
static_assert(FPH_LDS <= FPH_LDS_LIMIT, "fp head: LDS plan over one CU's LDS");

struct FphLayer {
    const float *W, *bias, *gamma, *beta, *rm, *rv;
    int ldw, cin, cout;
    float eps;
};

struct FphArgs {
    FphLayer L[FPH_MAX_NL + 1];                  // nl hidden layers, then the classifier
    const float *f1, *f2, *dist;
    const int* idx;
    float* out;
    unsigned char* mask;                         // nullable: (nl, rows, 128) ReLU decisions (pre-activation > 0)
    int ld1, d1, ldo, B, N, M, nl, ncls, rows;
};

// relu(acc + b) of four consecutive columns -> hi and lo bf16 (8 B each) at d and d + 32; returns the four
// decisions (value > 0) as bytes
__device__ __forceinline__ unsigned fph_relu_split4(__bf16* d, float a0, float a1, float a2, float a3, const float4 b) {
    const float z0 = a0 + b.x, z1 = a1 + b.y, z2 = a2 + b.z, z3 = a3 + b.w;
    const float v0 = fmaxf(z0, 0.f), v1 = fmaxf(z1, 0.f), v2 = fmaxf(z2, 0.f), v3 = fmaxf(z3, 0.f);
    const unsigned h0 = bx_pk(v0, v1), h1 = bx_pk(v2, v3);
    // v - float(hi): exact
    const unsigned l0 = bx_pk(v0 - __uint_as_float(h0 << 16), v1 - __uint_as_float(h0 & 0xffff0000u));
    const unsigned l1 = bx_pk(v2 - __uint_as_float(h1 << 16), v3 - __uint_as_float(h1 & 0xffff0000u));
    *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(d + 32) = make_uint2(l0, l1);
    return (z0 > 0.f ? 1u : 0u) | (z1 > 0.f ? 1u << 8 : 0u) | (z2 > 0.f ? 1u << 16 : 0u) | (z3 > 0.f ? 1u << 24 : 0u);
}

// One block = 4 waves = one tile of 128 consecutive rows of the (B N) row space; row >= rows re-reads the
// last row and is not written.
//
// LDS.  X: 5 slab images of 128 rows x 144 B.  The prologue fills nsl1 = ceil((D1 + 128) / 32) of them with
// the split planes of [f1 | interp], zero beyond D1 + 128; every hidden layer writes its 128 columns over
// images 0 .. 3 IN PLACE, behind the barrier that ends the layer's last step, and one more barrier
// publishes them.  W: two stages of 128 rows x 144 B, one 32-K slab of a layer's 128 columns each (the
// classifier: its four slabs of 32 zero-padded class columns, row = 32 slab + class).  Then the column
// scales and biases and the rows' interpolation records.
//
// Pipeline.  nsl1 + 4 (nl - 1) + 1 steps run through the two stages without draining between layers: step
// i + 1's weights (each thread owns two units of 8 consecutive K values of one column) are loaded from L2
// before step i's MFMAs and scaled by s, split and written to the other stage after them; one barrier per
// step, one more per hidden layer.
//
// Fragments.  The weight fragment goes first, so accumulator element 4 g + e of a 32 x 32 tile is (column
// 8 g + 4 h + e, row l32).  Hidden layers: wave w owns all 128 rows x columns 32 w .. 32 w + 31, four
// tiles (64 accumulator registers) sharing one weight fragment.  Classifier: wave w owns rows 32 w .. x
// the 32 class columns.
__global__ __launch_bounds__(256) void fp_head_infer_kernel(const FphArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fph_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int row0 = blockIdx.x * FPH_ROWS;      // rows < 2^31 - 128 (checked)
    const int nl = A.nl, d1 = A.d1, cin1 = d1 + FPH_W, nsl1 = (cin1 + 31) >> 5;
    __bf16* Xb = reinterpret_cast<__bf16*>(fph_lds);
    __bf16* Wd = Xb + FPH_NSLAB * FPH_IMG;
    float* sc = reinterpret_cast<float*>(Wd + 2 * FPH_STAGE);
    float* bs = sc + FPH_NCOEF;
    float* info = bs + FPH_NCOEF;

    // s (the arithmetic of bn_eval_coef_kernel, engine.hip) and the folded biases; classifier: 1 and bias
    for (int e = tid; e < FPH_NCOEF; e += 256) {
        const int l = e >> 7, n = e & (FPH_W - 1);
        float s = 0.f, bb = 0.f;
        if (l < nl) {
            const FphLayer& L = A.L[l];
            s = L.gamma[n] * (1.0f / sqrtf(L.rv[n] + L.eps));
            bb = s * ((L.bias ? L.bias[n] : 0.f) - L.rm[n]) + L.beta[n];
        } else if (l == FPH_MAX_NL && n < A.ncls) {
            s = 1.f;
            bb = A.L[nl].bias ? A.L[nl].bias[n] : 0.f;
        }
        sc[e] = s;
        bs[e] = bb;
    }
    // the rows' interpolation records: the three coarse rows (b M + idx, rows of f2) and the weights
    if (tid < FPH_ROWS) {
        const long long grow = min(row0 + tid, A.rows - 1);
        const int b = (int)(grow / A.N);
        PCS_DCHECK(grow >= 0 && grow < A.rows && b < A.B, "fp head idx / dist row %lld outside %d", grow, A.rows);
        int* ii = reinterpret_cast<int*>(info + tid * FPH_INFO);
        float w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int ix = A.idx[grow * 3 + k];
            PCS_DCHECK(ix >= 0 && ix < A.M, "fp head idx %d of row %lld outside %d coarse points", ix, grow, A.M);
            ii[k] = b * A.M + ix;
            w[k] = 1.0f / (A.dist[grow * 3 + k] + 1e-9f);
            info[tid * FPH_INFO + 3 + k] = w[k];
        }
        info[tid * FPH_INFO + 6] = (w[0] + w[1]) + w[2];
    }
    __syncthreads();               // the prologue reads info, load_w reads sc

    // channels c .. c + 3 of tile row r: the skip quad, the interpolated quad, or zeros past D1 + 128
    auto quad = [&](int r, int c) -> float4 {
        if (c < d1) {
            const float* p = A.f1 + (size_t)min(row0 + r, A.rows - 1) * A.ld1 + c;
            PCS_DCHECK_QUAD(p, A.f1, A.rows, A.ld1, d1, "fp head f1");
            return *reinterpret_cast<const float4*>(p);
        }
        if (c >= cin1) return make_float4(0.f, 0.f, 0.f, 0.f);
        const float* fi = info + r * FPH_INFO;
        const int* ii = reinterpret_cast<const int*>(fi);
        const float w0 = fi[3], w1 = fi[4], w2 = fi[5], nrm = fi[6];
        const float* p0 = A.f2 + (size_t)ii[0] * FPH_W + (c - d1);
        const float* p1 = A.f2 + (size_t)ii[1] * FPH_W + (c - d1);
        const float* p2 = A.f2 + (size_t)ii[2] * FPH_W + (c - d1);
        PCS_DCHECK_QUAD(p0, A.f2, (long long)A.B * A.M, FPH_W, FPH_W, "fp head f2");
        PCS_DCHECK_QUAD(p1, A.f2, (long long)A.B * A.M, FPH_W, FPH_W, "fp head f2");
        PCS_DCHECK_QUAD(p2, A.f2, (long long)A.B * A.M, FPH_W, FPH_W, "fp head f2");
        const float4 a = *reinterpret_cast<const float4*>(p0);
        const float4 q = *reinterpret_cast<const float4*>(p1);
        const float4 d = *reinterpret_cast<const float4*>(p2);
        float4 o;
        o.x = ((a.x * w0) / nrm + (q.x * w1) / nrm) + (d.x * w2) / nrm;
        o.y = ((a.y * w0) / nrm + (q.y * w1) / nrm) + (d.y * w2) / nrm;
        o.z = ((a.z * w0) / nrm + (q.z * w1) / nrm) + (d.z * w2) / nrm;
        o.w = ((a.w * w0) / nrm + (q.w * w1) / nrm) + (d.w * w2) / nrm;
        return o;
    };
    // consecutive threads take consecutive 8-K units of a row: a neighbour's 512-B row is read by 16 of them
    {
        const int upr = 4 * nsl1;
        for (int u = tid; u < FPH_ROWS * upr; u += 256) {
            const int r = u / upr, q = u - r * upr;
            uint4 hi, lo;
            bx_split8(quad(r, 8 * q), quad(r, 8 * q + 4), hi, lo);
            __bf16* d = Xb + (q >> 2) * FPH_IMG + r * FPH_LD + 8 * (q & 3);
            *reinterpret_cast<uint4*>(d) = hi;
            *reinterpret_cast<uint4*>(d + 32) = lo;
        }
    }

    const int nsteps = nsl1 + 4 * (nl - 1) + 1;
    float4 wa[2], wb[2];
    float sv[2];
    // step i: hidden layer l, K slab j (all 128 columns), or the classifier's four slabs of 32 columns
    auto load_w = [&](int i) {
        const bool cls = i == nsteps - 1;
        const int l = cls ? nl : i < nsl1 ? 0 : 1 + ((i - nsl1) >> 2);
        const int k0 = cls ? 0 : i < nsl1 ? 32 * i : 32 * ((i - nsl1) & 3);
        const FphLayer& L = A.L[l];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int unit = tid + 256 * u, r = unit >> 2;
            const int n = cls ? r & 31 : r;
            const int k = k0 + (cls ? 32 * (r >> 5) : 0) + 8 * (unit & 3);
            wa[u] = wb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            sv[u] = 0.f;
            if (n < L.cout) {
                const float* wp = L.W + (size_t)n * L.ldw + k;
                if (k < L.cin) {
                    PCS_DCHECK_QUAD(wp, L.W, L.cout, L.ldw, L.cin, "fp head W");
                    wa[u] = *reinterpret_cast<const float4*>(wp);
                }
                if (k + 4 < L.cin) {
                    PCS_DCHECK_QUAD(wp + 4, L.W, L.cout, L.ldw, L.cin, "fp head W");
                    wb[u] = *reinterpret_cast<const float4*>(wp + 4);
                }
                sv[u] = sc[(cls ? FPH_MAX_NL : l) * FPH_W + n];
            }
        }
    };
    auto store_w = [&](int stage) {
        __bf16* Ws = Wd + stage * FPH_STAGE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int unit = tid + 256 * u;
            const float s = sv[u];
            uint4 hi, lo;
            bx_split8(make_float4(s * wa[u].x, s * wa[u].y, s * wa[u].z, s * wa[u].w),
                      make_float4(s * wb[u].x, s * wb[u].y, s * wb[u].z, s * wb[u].w), hi, lo);
            __bf16* d = Ws + (unit >> 2) * FPH_LD + 8 * (unit & 3);
            *reinterpret_cast<uint4*>(d) = hi;
            *reinterpret_cast<uint4*>(d + 32) = lo;
        }
    };

    load_w(0);
    store_w(0);
    __syncthreads();               // X and stage 0

    const int fo = l32 * FPH_LD + 8 * h;                   // a lane's fragment offset inside a 32-row image
    f32x16 acc[4];
    int step = 0;
    for (int l = 0; l < nl; ++l) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x16{};
        const int ns = l == 0 ? nsl1 : 4;
        for (int j = 0; j < ns; ++j, ++step) {
            load_w(step + 1);                              // the classifier's step follows the last hidden one
            const __bf16* Xs = Xb + j * FPH_IMG + fo;
            const __bf16* Ws = Wd + (step & 1) * FPH_STAGE + 32 * wave * FPH_LD + fo;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 wh = *reinterpret_cast<const bf16x8*>(Ws + 16 * ks);
                const bf16x8 wl = *reinterpret_cast<const bf16x8*>(Ws + 16 * ks + 32);
                bf16x8 xh[4], xl[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    xh[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * FPH_LD + 16 * ks);
                    xl[i] = *reinterpret_cast<const bf16x8*>(Xs + 32 * i * FPH_LD + 16 * ks + 32);
                }
                // the three terms outermost, small terms first: four independent accumulators between two
                // MFMAs on the same one
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xl[i], acc[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xh[i], acc[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh[i], acc[i], 0, 0, 0);
            }
            store_w((step + 1) & 1);
            __syncthreads();
        }
        // every wave is past its last read of X: the layer's planes go over images 0 .. 3, image = wave
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = 32 * wave + 8 * g + 4 * h, r = 32 * i + l32;
                const float4 bv = *reinterpret_cast<const float4*>(bs + l * FPH_W + col);
                const unsigned m = fph_relu_split4(Xb + wave * FPH_IMG + r * FPH_LD + 8 * g + 4 * h, acc[i][4 * g],
                                                   acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3], bv);
                if (A.mask && row0 + r < A.rows) {
                    PCS_DCHECK(l < nl && col + 4 <= FPH_W, "fp head mask layer %d row %d col %d", l, row0 + r, col);
                    *reinterpret_cast<unsigned*>(A.mask + ((size_t)l * A.rows + row0 + r) * FPH_W + col) = m;
                }
            }
        __syncthreads();
    }

    // ---- classifier: class 8 g + 4 h + e of row 32 wave + l32
    f32x16 y = f32x16{};
    {
        const __bf16* Xs = Xb + 32 * wave * FPH_LD + fo;
        const __bf16* Ws = Wd + (step & 1) * FPH_STAGE + fo;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 xh = *reinterpret_cast<const bf16x8*>(Xs + s * FPH_IMG + 16 * ks);
                const bf16x8 xl = *reinterpret_cast<const bf16x8*>(Xs + s * FPH_IMG + 16 * ks + 32);
                const bf16x8 wh = *reinterpret_cast<const bf16x8*>(Ws + s * FPH_MAX_CLS * FPH_LD + 16 * ks);
                const bf16x8 wl = *reinterpret_cast<const bf16x8*>(Ws + s * FPH_MAX_CLS * FPH_LD + 16 * ks + 32);
                y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xl, y, 0, 0, 0);
                y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xh, y, 0, 0, 0);
                y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh, y, 0, 0, 0);
            }
    }
    const int row = row0 + 32 * wave + l32;
    if (row < A.rows) {
        const float* bc = bs + FPH_MAX_NL * FPH_W;
        float* op = A.out + (size_t)row * A.ldo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cls = 8 * (r >> 2) + 4 * h + (r & 3);
            if (cls < A.ncls) {
                PCS_DCHECK(row >= 0 && row < A.rows && cls < A.ldo, "fp head out row %d col %d outside %d x %d", row, cls,
                           A.rows, A.ncls);
                op[cls] = y[r] + bc[cls];
            }
        }
    }
}

// Every limit of the tail lives here (before any GPU work); fills the layers and sizes.
static int fph_check(const char* who, int B, int N, int M, int D1, int D2, const pcs_mlp_layer* layers, int nrec,
                     FphArgs& a) {
    PCS_CHECK_ARG(layers, "%s: null pointer", who);
    PCS_CHECK_ARG(nrec >= 2 && nrec <= FPH_MAX_NL + 1, "%s: %d records (1 .. %d hidden layers and the classifier)", who,
                  nrec, FPH_MAX_NL);
    PCS_CHECK_ARG(B >= 1 && N >= 1 && (long long)B * N < (1ll << 31) - FPH_ROWS, "%s: bad sizes B=%d N=%d", who, B, N);
    PCS_CHECK_ARG(M >= 3 && (long long)B * M < (1ll << 31), "%s: M %d coarse points (>= 3)", who, M);
    PCS_CHECK_ARG(D2 == FPH_W, "%s: D2 %d (the coarse features are %d wide)", who, D2, FPH_W);
    PCS_CHECK_ARG(D1 >= 0 && D1 % 4 == 0 && D1 <= FPH_MAX_D1, "%s: D1 %d (%% 4 == 0, 0 .. %d)", who, D1, FPH_MAX_D1);
    long long cin = D1 + D2;
    for (int l = 0; l < nrec; ++l) {
        const pcs_mlp_layer& R = layers[l];
        const bool last = l == nrec - 1;
        PCS_CHECK_ARG(R.W, "%s: layer %d null pointer", who, l);
        PCS_CHECK_ARG(R.use_batch == 0, "%s: layer %d BatchNorm is in training mode", who, l);
        if (last) {
            PCS_CHECK_ARG(!R.gamma && !R.beta && !R.run_mean && !R.run_var,
                          "%s: the last record carries a BatchNorm (the classifier is bias only)", who);
            PCS_CHECK_ARG(R.act == ACT_NONE, "%s: the last record's activation %lld (none)", who, (long long)R.act);
            PCS_CHECK_ARG(R.cout >= 1 && R.cout <= FPH_MAX_CLS, "%s: classes %lld (1 .. %d)", who, (long long)R.cout,
                          FPH_MAX_CLS);
        } else {
            PCS_CHECK_ARG(R.gamma && R.beta && R.run_mean && R.run_var, "%s: layer %d null pointer", who, l);
            PCS_CHECK_ARG(R.act == ACT_RELU, "%s: layer %d activation %lld (ReLU)", who, l, (long long)R.act);
            PCS_CHECK_ARG(R.cout == FPH_W, "%s: layer %d width %lld (the hidden layers are %d wide)", who, l,
                          (long long)R.cout, FPH_W);
        }
        PCS_CHECK_ARG(R.cin == cin && R.ldw >= cin && R.ldw < (1ll << 24), "%s: layer %d cin %lld ldw %lld (expected cin %lld)",
                      who, l, (long long)R.cin, (long long)R.ldw, cin);
        PCS_CHECK_ARG(R.ldw % 4 == 0 && (reinterpret_cast<uintptr_t>(R.W) & 15) == 0,
                      "%s: layer %d W must be 16-B aligned with ldw %% 4 == 0 (ldw %lld)", who, l, (long long)R.ldw);
        a.L[l] = FphLayer{R.W, R.bias, R.gamma, R.beta, R.run_mean, R.run_var, (int)R.ldw, (int)R.cin, (int)R.cout, (float)R.eps};
        cin = R.cout;
    }
    a.d1 = D1, a.B = B, a.N = N, a.M = M, a.nl = nrec - 1, a.ncls = (int)layers[nrec - 1].cout, a.rows = B * N;
    return 0;
}

}  // namespace pcs

using namespace pcs;

// Workspace bytes of pcs_fp_head_infer (none: *bytes = 0); non-zero (with a message) when the tail is not
// covered -- the coverage test of the bindings.  Sizes only: callable without a GPU.
PCS_API int pcs_fp_head_infer_workspace(int B, int N, int M, int D1, int D2, const pcs_mlp_layer* layers, int nrec,
                                        size_t* bytes) {
    PCS_CHECK_ARG(bytes, "pcs_fp_head_infer_workspace: null pointer");
    FphArgs a{};
    if (int rc = fph_check("pcs_fp_head_infer_workspace", B, N, M, D1, D2, layers, nrec, a)) return rc;
    *bytes = 0;
    return 0;
}

// Eval-mode FeaturePropagation + classifier.  f1 (B*N rows of D1 skip channels, row stride ld1; null with D1 =
// 0), f2 (B, M, D2 = 128) contiguous, idx / dist (B, N, 3) from pcs_knn_select; layers: nrec - 1 hidden
// records and the classifier's; out (B*N x classes, row stride ldo); mask: null, or (nrec - 1, B*N, 128)
// bytes that receive every hidden layer's ReLU decisions.  Reference: common.py:115-122, 238-243 and
// PointNetpp.py:46-47 under eval().
PCS_API int pcs_fp_head_infer(const float* f1, int ld1, int D1, const float* f2, int D2, const int32_t* idx,
                              const float* dist, int B, int N, int M, const pcs_mlp_layer* layers, int nrec, float* out,
                              int ldo, uint8_t* mask, void* stream) {
    FphArgs a{};
    if (int rc = fph_check("pcs_fp_head_infer", B, N, M, D1, D2, layers, nrec, a)) return rc;
    PCS_CHECK_ARG(f2 && idx && dist && out && (D1 == 0 || f1), "pcs_fp_head_infer: null pointer");
    PCS_CHECK_ARG(D1 == 0 || (ld1 % 4 == 0 && ld1 >= D1 && (reinterpret_cast<uintptr_t>(f1) & 15) == 0),
                  "pcs_fp_head_infer: ld1 %d (%% 4 == 0, >= D1 %d; f1 16-B aligned)", ld1, D1);
    PCS_CHECK_ARG((reinterpret_cast<uintptr_t>(f2) & 15) == 0, "pcs_fp_head_infer: f2 must be 16-B aligned");
    PCS_CHECK_ARG(((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(dist)) & 3) == 0,
                  "pcs_fp_head_infer: idx and dist must be 4-B aligned");
    PCS_CHECK_ARG(ldo >= a.ncls && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "pcs_fp_head_infer: ldo %d (>= classes %d)",
                  ldo, a.ncls);
    PCS_CHECK_ARG((reinterpret_cast<uintptr_t>(mask) & 3) == 0, "pcs_fp_head_infer: mask must be 4-B aligned");
    a.f1 = f1, a.f2 = f2, a.idx = idx, a.dist = dist, a.out = out, a.mask = mask;
    a.ld1 = ld1, a.ldo = ldo;
    hipStream_t st = as_stream(stream);
    // 134 KB of dynamic LDS: above the 64 KB default cap
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&fp_head_infer_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)FPH_LDS);
    (void)attr;
    const double rows = (double)a.rows;
    const double wts = (double)(D1 + D2) * FPH_W + (double)(a.nl - 1) * FPH_W * FPH_W + (double)FPH_W * a.ncls;
    {
        // compulsory bytes: idx, dist, the skip rows, the coarse features and the weights read once, out written
        ProbeScope pr(st, 2.0 * rows * wts, 4.0 * (rows * (6 + D1 + a.ncls) + (double)B * M * D2 + wts),
                      "pcs::fp_head_infer_kernel");
        hipLaunchKernelGGL(fp_head_infer_kernel, dim3((unsigned)((a.rows + FPH_ROWS - 1) / FPH_ROWS)), dim3(256), FPH_LDS,
                           st, a);
    }
    return launch_status("pcs_fp_head_infer");
}
