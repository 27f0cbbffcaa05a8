// Eval-mode SetAbstraction forward in one kernel (reference `SetAbstraction.forward` under
// model.eval(): group, common.py:37-71; MiniPointNet, common.py:125-150; reduce 'max',
// common.py:180-214): the inference / evaluation path of the PointNet++ family's grouped stacks.
//
// For group g = b C + c, neighbour j < K and p = idx[b, c, j]
//   x      = [ (xyz[b, p] - cent[b, c]) (/ r) , feats[b, p] ]           3 + D channels
//   a_l    = relu(W'_l a_(l-1) + b'_l)                                   l = 1 .. nl <= 3
//   out[g] = max_j a_nl
// with eval-mode BatchNorm folded into the conv while its weights are staged into LDS:
//   s = gamma / sqrt(running_var + eps),  W' = s o W,  b' = s o (bias - running_mean) + beta.
// Every row's full activation is computed before the max, so the sign of gamma needs no care
// (gamma == 0: W' = 0, b' = beta, out = relu(beta) exactly).  Only the pooled (B C, cout_nl) rows
// reach HBM: no grouped rows, no pre-BN Z, no argmax, no BN coefficients.
#include <algorithm>

#include "mlp_common.hpp"

namespace pcs {

constexpr int GMI_MAX_LAYERS = 3;
constexpr int GMI_MAX_WIDTH = 128;               // every layer width, and 3 + D <= GMI_MAX_WIDTH + 4
constexpr size_t GMI_LDS_LIMIT = 160 * 1024;     // one CU's LDS (gfx950)
constexpr int GMI_SB = 16;                       // weight loads in flight per thread while staging
constexpr int kGroupMlpBlocks = 256;             // persistent blocks: one per CU (the LDS need allows no second)

struct GmiLayer {
    const float *W, *bias, *gamma, *beta, *rm, *rv;
    int ldw, cin, cout;
    float eps;
};

// LDS map of a stack (floats).  Per layer: R = cout rounded to 32 folded weight rows of
// (cin rounded to 8) + 4 floats -- the row stride = 4 mod 8 keeps the 16 lanes of a ds_read_b128
// phase on distinct banks -- then R folded biases.  Then the activation ping-pong pair: tile A
// (the gathered input; layer 2's input) and tile B (layer 1's input), `rows` rows each with the same
// 4-mod-8 stride.
struct GmiPlan {
    int nl, rows, kin8, lda, ldb;
    int wofs[GMI_MAX_LAYERS], bofs[GMI_MAX_LAYERS], ldw[GMI_MAX_LAYERS], r32[GMI_MAX_LAYERS];
    int aofs, bofs_tile;
    size_t bytes;
};

static inline int up8(int n) { return (n + 7) & ~7; }

// The one place the LDS need (and so the 160 KB limit) is computed.  rows: 128 (4 waves) when it
// fits, else 64 (2 waves); bytes > GMI_LDS_LIMIT: the stack is not covered.
static GmiPlan gmi_plan(int kin, const int* widths, int nl) {
    GmiPlan P{};
    P.nl = nl;
    P.kin8 = up8(kin);
    int off = 0, cin = kin;
    for (int l = 0; l < nl; ++l) {
        P.ldw[l] = up8(cin) + 4;
        P.r32[l] = (widths[l] + 31) & ~31;
        P.wofs[l] = off;
        off += P.r32[l] * P.ldw[l];
        P.bofs[l] = off;
        off += P.r32[l];
        cin = widths[l];
    }
    P.lda = std::max(P.kin8, nl == 3 ? up8(widths[1]) : 0) + 4;
    P.ldb = nl >= 2 ? up8(widths[0]) + 4 : 0;
    for (int rows : {128, 64}) {
        P.rows = rows;
        P.aofs = off;
        P.bofs_tile = off + rows * P.lda;
        P.bytes = (size_t)(off + rows * (P.lda + P.ldb)) * sizeof(float);
        if (P.bytes <= GMI_LDS_LIMIT) break;
    }
    return P;
}

struct GmiArgs {
    GmiLayer L[GMI_MAX_LAYERS];
    GmiPlan P;
    const float *xyz, *feats, *cent;
    const int32_t* idx;
    int N, C, K, D, normalize, vec;   // vec: feats rows are read as float4 (D % 4 == 0, 16-B aligned)
    float r;
    long long G;                      // groups B C
    float* out;
};

// One layer for this wave's 32 rows: acc (32 x 32 NT) = act (32 x cin8) . W'^T on
// v_mfma_f32_32x32x2_f32.  Both fragments have the same shape -- lane l32 = the tile's row (a point
// row of `in`, a folded weight row of Wl), lane half h = channels 8 s + 4 h .. + 3, one ds_read_b128
// each -- so the operand order picks the accumulator's orientation:
//   !LAST  weight fragment first: element 4 g + e of tile j = (column 32 j + 8 g + 4 h + e, row l32),
//          four consecutive columns of one row per lane, so b' + ReLU + the write into the other
//          activation tile are float4;
//   LAST   activation fragment first: element r of tile j = (row (r & 3) + 8 (r >> 2) + 4 h, column
//          32 j + l32), so the max over a group's rows is in-lane plus one __shfl_xor(.., 32): K = 32
//          pools all 16 elements, K = 16 elements 0..7 (rows 0..15) and 8..15 (rows 16..31) apart.
//          max_j relu(a_j + b') = relu(max_j a_j + b') exactly (rounding is monotone).
template <int NT, bool LAST>
__device__ __forceinline__ void gmi_layer(const float* __restrict__ in, int ldi, const float* __restrict__ Wl,
                                          const float* __restrict__ bl, int ldw, int cin8, int cout, float* __restrict__ nxt,
                                          int ldn, int l32, int h, int K, long long grp0, long long G,
                                          float* __restrict__ out) {
    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x16{};
    const float* ar = in + l32 * ldi + 4 * h;
    const float* wr = Wl + l32 * ldw + 4 * h;
    for (int c = 0; c < cin8; c += 8) {
        const float4 xa = *reinterpret_cast<const float4*>(ar + c);
        float4 wa[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) wa[j] = *reinterpret_cast<const float4*>(wr + 32 * j * ldw + c);
        // NT independent accumulators between two MFMAs on the same one
#define GMI_MMA(E)                                                                                       \
    _Pragma("unroll") for (int j = 0; j < NT; ++j) acc[j] =                                              \
        LAST ? __builtin_amdgcn_mfma_f32_32x32x2f32(xa.E, wa[j].E, acc[j], 0, 0, 0)                      \
             : __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j].E, xa.E, acc[j], 0, 0, 0);
        GMI_MMA(x) GMI_MMA(y) GMI_MMA(z) GMI_MMA(w)
#undef GMI_MMA
    }
    if constexpr (!LAST) {
        const int cout8 = (cout + 7) & ~7;        // the next layer's K range: columns cout .. cout8 get relu(0 + 0)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = 32 * j + 8 * g + 4 * h;
                if (n >= cout8) continue;
                const float4 b = *reinterpret_cast<const float4*>(bl + n);
                *reinterpret_cast<float4*>(nxt + l32 * ldn + n) =
                    make_float4(fmaxf(acc[j][4 * g] + b.x, 0.f), fmaxf(acc[j][4 * g + 1] + b.y, 0.f),
                                fmaxf(acc[j][4 * g + 2] + b.z, 0.f), fmaxf(acc[j][4 * g + 3] + b.w, 0.f));
            }
    } else {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float lo = acc[j][0], hi = acc[j][8];
#pragma unroll
            for (int r = 1; r < 8; ++r) {
                lo = fmaxf(lo, acc[j][r]);
                hi = fmaxf(hi, acc[j][8 + r]);
            }
            lo = fmaxf(lo, __shfl_xor(lo, 32, 64));
            hi = fmaxf(hi, __shfl_xor(hi, 32, 64));
            const int n = 32 * j + l32;
            // K = 32: one group per wave, stored by lane half 0; K = 16: half h stores group h
            const float m = K == 32 ? fmaxf(lo, hi) : (h ? hi : lo);
            const long long g = K == 32 ? grp0 : 2 * grp0 + h;
            if (n < cout && g < G && (K == 16 || h == 0)) {
                PCS_DCHECK(g >= 0 && g * cout + n < G * cout, "group mlp infer out row %lld col %d outside %lld x %d", g, n,
                           G, cout);
                out[g * cout + n] = fmaxf(m + bl[n], 0.f);
            }
        }
    }
}

template <bool LAST>
__device__ __forceinline__ void gmi_layer_nt(int nt, const float* in, int ldi, const float* Wl, const float* bl, int ldw,
                                             int cin8, int cout, float* nxt, int ldn, int l32, int h, int K,
                                             long long grp0, long long G, float* out) {
    switch (nt) {
    case 1: gmi_layer<1, LAST>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, l32, h, K, grp0, G, out); break;
    case 2: gmi_layer<2, LAST>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, l32, h, K, grp0, G, out); break;
    case 3: gmi_layer<3, LAST>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, l32, h, K, grp0, G, out); break;
    default: gmi_layer<4, LAST>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, l32, h, K, grp0, G, out); break;
    }
}

// One persistent block of rows / 32 waves per CU.  Prologue: every layer's folded weights and biases
// go into LDS once (W' and b' formed while staging: no fold launch, no folded copy in HBM).  Then
// the block sweeps row tiles of `rows` rows = rows / K whole groups; wave w owns rows 32 w .. + 31 of
// both activation tiles through all layers, and its two threads per row gather that row:
//   thread (row, parity) holds items q = parity, parity + 2, ..: q = 0 the row's xyz and its
//   centroid (12 B each), q >= 1 the feats quad q - 1 (one float4 when the rows allow, else scalars).
// The gather is software-pipelined two deep: a tile's index is loaded two tiles ahead and its rows one
// tile ahead, right after the previous tile's registers were written to LDS, so they are in flight
// across that tile's whole layer loop (NQ = items per thread, all in registers: one wave per SIMD
// owns its 512).  Channels 3 + D .. kin8 are written as zeros each tile (tile A is also layer 2's
// input).  Tile order: edgeconv_fwd_kernel's XCD-aware ranges -- blocks b, b + 8, .. sweep one
// contiguous range of groups, so an XCD gathers about one cloud's features out of its own L2.
template <int NQ>
__global__ __launch_bounds__(256) void group_mlp_infer_kernel(const GmiArgs A) {
    extern __shared__ __attribute__((aligned(16))) float gmi_lds[];
    const GmiPlan& P = A.P;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;

    // BN's scale s (the arithmetic of bn_eval_coef_kernel, engine.hip) into scratch at the head of tile A,
    // b' into its place; rows at or beyond cout are zero
    for (int l = 0; l < P.nl; ++l) {
        const GmiLayer& L = A.L[l];
        for (int n = tid; n < P.r32[l]; n += nth) {
            float s = 0.f, b = 0.f;
            if (n < L.cout) {
                s = L.gamma[n] * (1.0f / sqrtf(L.rv[n] + L.eps));
                b = s * ((L.bias ? L.bias[n] : 0.f) - L.rm[n]) + L.beta[n];
            }
            gmi_lds[P.aofs + GMI_MAX_WIDTH * l + n] = s;
            gmi_lds[P.bofs[l] + n] = b;
        }
    }
    __syncthreads();
    // W' = s o W, GMI_SB loads in flight per thread (one at a time, the 72 KB of an SA2 stack cost
    // ~48 us per block); channels at or beyond cin are zero, every load lies in W's (cout - 1) ldw + cin floats
    for (int l = 0; l < P.nl; ++l) {
        const GmiLayer& L = A.L[l];
        float* Ws = gmi_lds + P.wofs[l];
        const float* sv = gmi_lds + P.aofs + GMI_MAX_WIDTH * l;
        const int ldw = P.ldw[l], total = P.r32[l] * ldw;
        for (int e0 = tid; e0 < total; e0 += GMI_SB * nth) {
            float w[GMI_SB];
#pragma unroll
            for (int u = 0; u < GMI_SB; ++u) {
                const int e = e0 + u * nth, n = e / ldw, c = e - n * ldw;
                w[u] = e < total && n < L.cout && c < L.cin ? L.W[(size_t)n * L.ldw + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < GMI_SB; ++u) {
                const int e = e0 + u * nth;
                if (e < total) Ws[e] = sv[e / ldw] * w[u];
            }
        }
    }

    float* tA = gmi_lds + P.aofs + 32 * wave * P.lda;       // this wave's 32 rows of either tile
    float* tB = gmi_lds + P.bofs_tile + 32 * wave * P.ldb;
    const int rows = P.rows, K = A.K, D = A.D, N = A.N;
    const long long M = A.G * K;
    const long long tiles = (M + rows - 1) / rows;
    const int nx = gridDim.x % 8 == 0 ? 8 : 1;
    const int xcd = blockIdx.x % nx, lb = blockIdx.x / nx, nlb = gridDim.x / nx;
    const long long tx = (tiles + nx - 1) / nx;
    const long long t0 = (long long)xcd * tx, t1 = min(tiles, t0 + tx);
    const int row = tid >> 1, par = tid & 1;
    const int nq = 1 + (P.kin8 - 3 + 3) / 4;                 // items per row: xyz + quads up to channel kin8

    // a tile's row of this thread (the ragged tail re-reads row M - 1; its groups are never stored)
    auto row_of = [&](long long t) { return min(t * rows + row, M - 1); };
    auto load_idx = [&](long long t) { return t < t1 ? min(max(A.idx[row_of(t)], 0), N - 1) : 0; };
    float4 v[NQ];
    float cx = 0.f, cy = 0.f, cz = 0.f;
    auto load_rows = [&](long long t, int p) {
        if (t >= t1) return;
        const long long g = row_of(t) / K;
        const long long pb = (g / A.C) * N + p;
        PCS_DCHECK(p >= 0 && p < N && g < A.G, "group mlp infer point %d of group %lld outside %d x %lld", p, g, N, A.G);
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int q = par + 2 * u;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q == 0) {
                x = make_float4(A.xyz[pb * 3], A.xyz[pb * 3 + 1], A.xyz[pb * 3 + 2], 0.f);
                cx = A.cent[g * 3], cy = A.cent[g * 3 + 1], cz = A.cent[g * 3 + 2];
            } else if (q < nq) {
                const int c = 4 * (q - 1);
                const float* f = A.feats + pb * D + c;
                if (A.vec) {
                    if (c < D) x = *reinterpret_cast<const float4*>(f);       // D % 4 == 0: the quad is inside the row
                } else {
                    x.x = c + 0 < D ? f[0] : 0.f;
                    x.y = c + 1 < D ? f[1] : 0.f;
                    x.z = c + 2 < D ? f[2] : 0.f;
                    x.w = c + 3 < D ? f[3] : 0.f;
                }
            }
            v[u] = x;
        }
    };
    // registers -> tile A: the arithmetic of group_fwd_q_kernel (fp32 subtract, then a true division)
    auto write_rows = [&]() {
        float* dst = gmi_lds + P.aofs + row * P.lda;
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int q = par + 2 * u;
            if (q == 0) {
                float x = v[u].x - cx, y = v[u].y - cy, z = v[u].z - cz;
                if (A.normalize) x = x / A.r, y = y / A.r, z = z / A.r;
                dst[0] = x, dst[1] = y, dst[2] = z;
            } else if (q < nq) {
                const int c = 3 + 4 * (q - 1);
                if (c + 0 < P.kin8) dst[c + 0] = v[u].x;
                if (c + 1 < P.kin8) dst[c + 1] = v[u].y;
                if (c + 2 < P.kin8) dst[c + 2] = v[u].z;
                if (c + 3 < P.kin8) dst[c + 3] = v[u].w;
            }
        }
    };

    long long t = t0 + lb;
    int pn = load_idx(t + nlb);
    load_rows(t, load_idx(t));
    const int nl = P.nl;
    for (; t < t1; t += nlb) {
        __syncthreads();                     // the staged weights (first tile); the previous tile's readers of tile A
        write_rows();
        __syncthreads();
        load_rows(t + nlb, pn);              // in flight across the layer loop
        pn = load_idx(t + 2 * nlb);
        const long long grp0 = t * (rows / 32) + wave;       // this wave's 32-row block, in units of 32 rows
        const float* W0 = gmi_lds + P.wofs[0];
        const float* b0 = gmi_lds + P.bofs[0];
        if (nl == 1) {
            gmi_layer_nt<true>(P.r32[0] / 32, tA, P.lda, W0, b0, P.ldw[0], P.kin8, A.L[0].cout, nullptr, 0, l32, h, K, grp0,
                               A.G, A.out);
            continue;
        }
        gmi_layer_nt<false>(P.r32[0] / 32, tA, P.lda, W0, b0, P.ldw[0], P.kin8, A.L[0].cout, tB, P.ldb, l32, h, K, grp0, A.G,
                            nullptr);
        __syncthreads();
        const float* W1 = gmi_lds + P.wofs[1];
        const float* b1 = gmi_lds + P.bofs[1];
        if (nl == 2) {
            gmi_layer_nt<true>(P.r32[1] / 32, tB, P.ldb, W1, b1, P.ldw[1], P.ldw[1] - 4, A.L[1].cout, nullptr, 0, l32, h, K,
                               grp0, A.G, A.out);
            continue;
        }
        gmi_layer_nt<false>(P.r32[1] / 32, tB, P.ldb, W1, b1, P.ldw[1], P.ldw[1] - 4, A.L[1].cout, tA, P.lda, l32, h, K,
                            grp0, A.G, nullptr);
        __syncthreads();
        gmi_layer_nt<true>(P.r32[2] / 32, tA, P.lda, gmi_lds + P.wofs[2], gmi_lds + P.bofs[2], P.ldw[2], P.ldw[2] - 4,
                           A.L[2].cout, nullptr, 0, l32, h, K, grp0, A.G, A.out);
    }
}

template <int NQ>
static void gmi_launch(int grid, int threads, size_t lds, hipStream_t st, const GmiArgs& a) {
    // up to 160 KB of dynamic LDS: above the 64 KB default cap
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&group_mlp_infer_kernel<NQ>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)GMI_LDS_LIMIT);
    (void)attr;
    hipLaunchKernelGGL(group_mlp_infer_kernel<NQ>, dim3(grid), dim3(threads), lds, st, a);
}

// shape checks shared by the two entry points; 0 = covered
static int gmi_check(const char* who, int kin, const int* widths, int nl, int K) {
    PCS_CHECK_ARG(nl >= 1 && nl <= GMI_MAX_LAYERS, "%s: %d layers (1 .. %d)", who, nl, GMI_MAX_LAYERS);
    PCS_CHECK_ARG(K == 16 || K == 32, "%s: K=%d (16 or 32)", who, K);
    PCS_CHECK_ARG(kin >= 4 && kin <= GMI_MAX_WIDTH + 4, "%s: 3 + D = %d (4 .. %d)", who, kin, GMI_MAX_WIDTH + 4);
    for (int l = 0; l < nl; ++l)
        PCS_CHECK_ARG(widths[l] >= 4 && widths[l] % 4 == 0 && widths[l] <= GMI_MAX_WIDTH,
                      "%s: layer %d width %d (%% 4 == 0, <= %d)", who, l, widths[l], GMI_MAX_WIDTH);
    const GmiPlan P = gmi_plan(kin, widths, nl);
    PCS_CHECK_ARG(P.bytes <= GMI_LDS_LIMIT, "%s: the stack needs %zu B of LDS (limit %zu)", who, P.bytes, GMI_LDS_LIMIT);
    return 0;
}

}  // namespace pcs

using namespace pcs;

// LDS bytes of pcs_group_mlp_infer for a stack of nl layers of `widths` on 3 + D = kin channels pooled
// over K; non-zero (with a message) when the shape is not covered -- the coverage test of the bindings.
PCS_API int pcs_group_mlp_infer_lds(int kin, const int* widths, int nl, int K, size_t* bytes) {
    PCS_CHECK_ARG(widths && bytes, "pcs_group_mlp_infer_lds: null pointer");
    if (int rc = gmi_check("pcs_group_mlp_infer_lds", kin, widths, nl, K)) return rc;
    *bytes = gmi_plan(kin, widths, nl).bytes;
    return 0;
}

// Eval-mode grouped MLP + max-pool.  xyz (B, N, 3), feats (B, N, D), cent (B, C, 3), idx (B, C, K)
// int32 per-cloud neighbour table; layers: nl pcs_mlp_layer records (W .. slope; eval mode, ReLU);
// out (B*C, cout_nl).  Reference: common.py:37-71, 125-150, 180-214 under eval().
PCS_API int pcs_group_mlp_infer(const float* xyz, const float* feats, const float* cent, const int32_t* idx, int B,
                                int N, int C, int K, int D, float r, int normalize, const pcs_mlp_layer* layers, int nl,
                                float* out, void* stream) {
    PCS_CHECK_ARG(B >= 1 && N >= 1 && C >= 1 && D >= 1, "pcs_group_mlp_infer: bad sizes B=%d N=%d C=%d D=%d", B, N, C, D);
    PCS_CHECK_ARG(xyz && feats && cent && idx && layers && out, "pcs_group_mlp_infer: null pointer");
    PCS_CHECK_ARG(nl >= 1 && nl <= GMI_MAX_LAYERS, "pcs_group_mlp_infer: %d layers (1 .. %d)", nl, GMI_MAX_LAYERS);
    int widths[GMI_MAX_LAYERS];
    GmiArgs a{};
    int cin = 3 + D;
    for (int l = 0; l < nl; ++l) {
        const pcs_mlp_layer& R = layers[l];
        PCS_CHECK_ARG(R.W && R.gamma && R.beta && R.run_mean && R.run_var, "pcs_group_mlp_infer: layer %d null pointer", l);
        PCS_CHECK_ARG(R.use_batch == 0, "pcs_group_mlp_infer: layer %d BatchNorm is in training mode", l);
        PCS_CHECK_ARG(R.act == 0, "pcs_group_mlp_infer: layer %d activation %lld (ReLU only)", l, (long long)R.act);
        PCS_CHECK_ARG(R.cin == cin && R.ldw >= cin, "pcs_group_mlp_infer: layer %d cin %lld ldw %lld (expected cin %d)", l,
                      (long long)R.cin, (long long)R.ldw, cin);
        PCS_CHECK_ARG(R.cout >= 4 && R.cout <= GMI_MAX_WIDTH, "pcs_group_mlp_infer: layer %d width %lld (%% 4 == 0, <= %d)",
                      l, (long long)R.cout, GMI_MAX_WIDTH);
        widths[l] = (int)R.cout;
        a.L[l] = GmiLayer{R.W, R.bias, R.gamma, R.beta, R.run_mean, R.run_var, (int)R.ldw, cin, (int)R.cout, (float)R.eps};
        cin = (int)R.cout;
    }
    if (int rc = gmi_check("pcs_group_mlp_infer", 3 + D, widths, nl, K)) return rc;
    PCS_CHECK_ARG(!normalize || r > 0.f, "pcs_group_mlp_infer: radius %g with normalised grouping", (double)r);
    const long long G = (long long)B * C;
    PCS_CHECK_ARG(G * K < (1ll << 31) && (long long)B * N < (1ll << 31), "pcs_group_mlp_infer: too many rows");
    a.P = gmi_plan(3 + D, widths, nl);
    a.xyz = xyz, a.feats = feats, a.cent = cent, a.idx = idx;
    a.N = N, a.C = C, a.K = K, a.D = D, a.normalize = normalize, a.r = r, a.G = G, a.out = out;
    a.vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(feats) & 15) == 0;
    hipStream_t st = as_stream(stream);
    const long long tiles = (G * K + a.P.rows - 1) / a.P.rows;
    const int grid = (int)std::min<long long>(kGroupMlpBlocks, tiles >= 8 ? (tiles + 7) / 8 * 8 : tiles);
    const int threads = 2 * a.P.rows;
    const int need = ((1 + (a.P.kin8 - 3 + 3) / 4) + 1) / 2;      // gather items per thread
    double flops = 0.0;
    for (int l = 0; l < nl; ++l) flops += 2.0 * (double)G * K * a.L[l].cin * a.L[l].cout;
    // compulsory bytes: the points' coordinates and features, the centroids and idx read once, out written
    ProbeScope pr(st, flops, 4.0 * ((double)B * N * (3 + D) + 3.0 * G + (double)G * K + (double)G * widths[nl - 1]),
                  "pcs::group_mlp_infer_kernel<%d>", need <= 3 ? 3 : need <= 6 ? 6 : need <= 10 ? 10 : 18);
    if (need <= 3) gmi_launch<3>(grid, threads, a.P.bytes, st, a);
    else if (need <= 6) gmi_launch<6>(grid, threads, a.P.bytes, st, a);
    else if (need <= 10) gmi_launch<10>(grid, threads, a.P.bytes, st, a);
    else gmi_launch<18>(grid, threads, a.P.bytes, st, a);
    return launch_status("pcs_group_mlp_infer");
}
