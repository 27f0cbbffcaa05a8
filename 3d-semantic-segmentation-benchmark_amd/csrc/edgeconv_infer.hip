// Eval-mode EdgeConv forward (reference `EdgeConv` under model.eval(), models/dgcnn/dgcnn.py:60-77
// with `get_graph_feature`, dgcnn.py:24-57): the inference / evaluation path of DGCNN.
//
// With W = [W1 | W2] (Cout x 2C) the edge value is z_(i,j) = W1 x_j + (W2 - W1) x_i (edgeconv.hip),
// and eval-mode BatchNorm is an affine map known before the launch:
//   s = gamma / sqrt(running_var + eps),  t = beta - running_mean s
// LeakyReLU with slope >= 0 is non-decreasing, so with
//   U = s o (X W1^T)            V = s o (X (W2 - W1)^T) + t
//   out_i = max_j act(s z_(i,j) + t) = act(max_j U_j + V_i)
// s is folded into U, so the reduction is a plain max for every sign of gamma (s < 0 turns the
// min over Y into a max over U; s == 0 gives U = 0, V = t and out = act(t)).  No statistics, no
// argmax, nothing saved: one point-transform GEMM and one gather-max.
//
//   edgeconv_infer_point_kernel   (U | V) = X [W1 ; W2 - W1]^T through s, t: one pass over X
//   edgeconv_infer_gather_kernel  out_i = act(max_j U_j + V_i), and its second copy out2
#include "mlp_common.hpp"

namespace pcs {

constexpr int EI_ROWS = 128;             // point rows per tile of the point transform (32 per wave)
constexpr int EI_KB = 8;                 // K steps (8 channels each) whose X fragments are in flight
constexpr int EI_FB = 8;                 // neighbour rows per gather batch (EC_FB of edgeconv.hip)
constexpr int kInferPointBlocks = 512;   // persistent blocks of the point transform (2 per CU)
constexpr int kInferGatherBlocks = 1024;

// LDS of the point transform: NT*32 folded weight rows of (C rounded to 8) + 4 floats, then s, t
static size_t infer_lds_bytes(int NT, int C, int Cout) {
    return ((size_t)NT * 32 * (((C + 7) & ~7) + 4) + 2 * (size_t)Cout) * sizeof(float);
}

// One block = 4 waves; it keeps ALL 2 Cout folded weight rows in LDS (staged once, W2 - W1 formed
// while staging) and sweeps 128-row tiles of X, 32 rows per wave, so X is read from HBM exactly once
// and there is no fold launch or folded weight copy.  NT = 32-column tiles of the (U | V) row
// (2 Cout <= 32 NT), accumulated at most 4 at a time from the same X registers (all 8 at once:
// 428 registers, one block per CU, 54.5 us for the 65536 x 64 -> 2 x 128 layer against 42.8 us in
// two passes).  v_mfma_f32_32x32x2_f32 computes the TRANSPOSED product: the A operand is the
// weight fragment (lane l32 = folded row 32 j + l32, lane half h = channels 8 s + 4 h .. + 3, one
// ds_read_b128; the row stride = 4 mod 8 floats keeps the 16 lanes of a read phase on distinct
// banks) and the B operand the X fragment, loaded from global memory straight into that layout
// (lane l32 = point row, the same channel quad: a 32-B run per row and instruction).  Accumulator
// element 4 g + e of tile j is then (column 32 j + 8 g + 4 h + e, row l32): four consecutive
// columns of one point per lane, so the epilogue's s / t and its stores are float4 with no LDS
// transpose.
template <int NT>
__global__ __launch_bounds__(256) void edgeconv_infer_point_kernel(
    const float* __restrict__ X, int ldx, int C, int M, const float* __restrict__ W, int Cout,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
    const float* __restrict__ rv, float eps, float* __restrict__ U, float* __restrict__ V) {
    extern __shared__ __attribute__((aligned(16))) float ei_lds[];
    constexpr int NA = NT < 4 ? NT : 4;       // column tiles accumulated at a time
    const int Cp = (C + 7) & ~7, LDW = Cp + 4, KS = Cp / 8, cq = Cp / 4;
    float* Ws = ei_lds;                       // [NT * 32][LDW]
    float* sc = Ws + NT * 32 * LDW;           // [Cout] s, then [Cout] t
    float* tc = sc + Cout;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;

    // folded weight rows: n < Cout -> W1 row n, n < 2 Cout -> (W2 - W1) row n - Cout, else zero;
    // channels at or beyond C are zero.  Every load lies in W's Cout x 2C floats.
    for (int e = tid; e < NT * 32 * cq; e += 256) {
        const int n = e / cq, c = 4 * (e - n * cq);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < 2 * Cout && c < C) {
            const bool second = n >= Cout;
            const float* w1 = W + (size_t)(second ? n - Cout : n) * 2 * C + c;
            PCS_DCHECK(w1 - W + C + min(4, C - c) <= (long long)Cout * 2 * C, "edgeconv infer W row %d col %d outside %d x %d",
                       n, c, Cout, 2 * C);
            if (C % 4 == 0) {
                v = *reinterpret_cast<const float4*>(w1);
                if (second) {
                    const float4 w2 = *reinterpret_cast<const float4*>(w1 + C);
                    v = make_float4(__fsub_rn(w2.x, v.x), __fsub_rn(w2.y, v.y), __fsub_rn(w2.z, v.z),
                                    __fsub_rn(w2.w, v.w));
                }
            } else {                          // C < 4 (unaligned 2C-float rows): scalar loads
                float q[4] = {0.f, 0.f, 0.f, 0.f};
                for (int i = 0; i < C; ++i) q[i] = second ? __fsub_rn(w1[C + i], w1[i]) : w1[i];
                v = make_float4(q[0], q[1], q[2], q[3]);
            }
        }
        *reinterpret_cast<float4*>(Ws + n * LDW + c) = v;
    }
    // eval-mode BN coefficients (the arithmetic of bn_eval_coef_kernel, engine.hip)
    for (int n = tid; n < Cout; n += 256) {
        const float inv = 1.0f / sqrtf(rv[n] + eps);
        const float s = gamma[n] * inv;
        sc[n] = s;
        tc[n] = beta[n] - rm[n] * s;
    }
    __syncthreads();

    const int tiles = (M + EI_ROWS - 1) / EI_ROWS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row = tile * EI_ROWS + 32 * wave + l32;
        const float* xr = X + (size_t)min(row, M - 1) * ldx;      // the tail's rows re-read row M - 1
        // this lane's channel quads of up to EI_KB steps from s0, all issued before their first MFMA; a
        // quad at or beyond C is zero (C < 4: per element -- xyz zero-extended to one K = 4 step)
        auto load_x = [&](int s0, float4* xb) {
#pragma unroll
            for (int u = 0; u < EI_KB; ++u) {
                const int c = 8 * (s0 + u) + 4 * h;
                const bool in = c < C;
                PCS_DCHECK(!in || c + 4 <= ((C + 3) & ~3), "edgeconv infer X row %d col %d outside %d x %d", row, c, M, C);
                float4 v = *reinterpret_cast<const float4*>(xr + (in ? c : 0));
                v.x = c + 0 < C ? v.x : 0.f;
                v.y = c + 1 < C ? v.y : 0.f;
                v.z = c + 2 < C ? v.z : 0.f;
                v.w = c + 3 < C ? v.w : 0.f;
                xb[u] = v;
            }
        };
        float4 x0[EI_KB];                     // steps 0 .. EI_KB - 1 (all of C <= 64), shared by the column passes
        load_x(0, x0);
        // NA column tiles (128 columns) per pass: 64 accumulator registers, two blocks per CU
        for (int j0 = 0; j0 < NT; j0 += NA) {
            f32x16 acc[NA];
#pragma unroll
            for (int j = 0; j < NA; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            auto mma = [&](int s0, const float4* xb) {
#pragma unroll
                for (int u = 0; u < EI_KB; ++u) {
                    if (s0 + u >= KS) break;
                    float4 wa[NA];
#pragma unroll
                    for (int j = 0; j < NA; ++j)
                        wa[j] = *reinterpret_cast<const float4*>(Ws + (32 * (j0 + j) + l32) * LDW + 8 * (s0 + u) + 4 * h);
                    // NA independent accumulators between two MFMAs on the same one
#pragma unroll
                    for (int j = 0; j < NA; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j].x, xb[u].x, acc[j], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < NA; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j].y, xb[u].y, acc[j], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < NA; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j].z, xb[u].z, acc[j], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < NA; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j].w, xb[u].w, acc[j], 0, 0, 0);
                }
            };
            mma(0, x0);
            for (int s0 = EI_KB; s0 < KS; s0 += EI_KB) {      // C > 64: the later steps are re-read per pass (L1 / L2)
                float4 xb[EI_KB];
                load_x(s0, xb);
                mma(s0, xb);
            }
            if (row < M) {
#pragma unroll
                for (int j = 0; j < NA; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int n = 32 * (j0 + j) + 8 * g + 4 * h;
                        if (n >= 2 * Cout) continue;
                        const bool second = n >= Cout;              // Cout % 4 == 0: a quad is all U or all V
                        const int c = second ? n - Cout : n;
                        PCS_DCHECK(c + 4 <= Cout, "edgeconv infer U/V row %d col %d outside %d x %d", row, c, M, Cout);
                        const float4 s = *reinterpret_cast<const float4*>(sc + c);
                        float4 o = make_float4(s.x * acc[j][4 * g], s.y * acc[j][4 * g + 1], s.z * acc[j][4 * g + 2],
                                               s.w * acc[j][4 * g + 3]);
                        if (second) {
                            const float4 t = *reinterpret_cast<const float4*>(tc + c);
                            o = make_float4(o.x + t.x, o.y + t.y, o.z + t.z, o.w + t.w);
                        }
                        *reinterpret_cast<float4*>((second ? V : U) + (size_t)row * Cout + c) = o;
                    }
            }
        }
    }
}

// Cout / 4 lanes share one point, a channel quad each (a wave: 4 points at Cout = 64, 2 at 128), so a
// neighbour's U row is one coalesced 256-B / 512-B read.  Per batch of EI_FB neighbours the first
// EI_FB lanes of the point's lane group load one index each (clamped to the cloud as the training
// kernel does) and the group reads them by __shfl; the next batch's indices are loaded before this
// batch's rows, and a batch's rows are all issued before its max.  (Fewer than EI_FB lanes per point,
// Cout < 32: every lane loads the indices itself.)  Point order: edgeconv_fwd_kernel's XCD-aware
// ranges -- blocks b, b + 8, ... sweep one contiguous range of points together, so an XCD gathers
// the U rows of about one cloud (1 MB at N = 4096, Cout = 64) out of its own L2.
__global__ __launch_bounds__(256) void edgeconv_infer_gather_kernel(const float* __restrict__ U,
                                                                    const float* __restrict__ V,
                                                                    const int32_t* __restrict__ idx, int N, int k,
                                                                    int Cout, long long G, float slope,
                                                                    float* __restrict__ out, float* __restrict__ out2,
                                                                    int ld2) {
    const int tq = Cout / 4;                       // lanes per point
    const int gpw = 64 / tq;                       // points per wave (lanes past gpw * tq idle)
    const int pb = 4 * gpw;                        // points per block pass
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / tq, lig = lane - grp * tq, base = grp * tq;
    const int c = 4 * lig;
    const bool shfl = tq >= EI_FB;
    const int nx = gridDim.x % 8 == 0 ? 8 : 1;
    const int xcd = blockIdx.x % nx, lb = blockIdx.x / nx, nl = gridDim.x / nx;
    const long long Gx = (G + nx - 1) / nx;
    const long long gx0 = (long long)xcd * Gx, gx1 = min(G, gx0 + Gx);
    if (grp >= gpw) return;
    // the lanes of a group share g, so they run the loop (and its shuffles) together
    for (long long g = gx0 + (long long)lb * pb + wave * gpw + grp; g < gx1; g += (long long)nl * pb) {
        const long long cloud = (g / N) * N;
        const int32_t* nb = idx + g * k;
        const float4 vi = *reinterpret_cast<const float4*>(V + g * Cout + c);
        float mx[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        auto load_idx = [&](int k0) { return lig < EI_FB && k0 + lig < k ? min(max(nb[k0 + lig], 0), N - 1) : 0; };
        int jn = shfl ? load_idx(0) : 0;
        for (int k0 = 0; k0 < k; k0 += EI_FB) {
            const int jl = jn;
            if (shfl && k0 + EI_FB < k) jn = load_idx(k0 + EI_FB);
            float4 ub[EI_FB];
#pragma unroll
            for (int u = 0; u < EI_FB; ++u) {
                int j;
                if (shfl) j = __shfl(jl, base + u, 64);
                else j = k0 + u < k ? min(max(nb[k0 + u], 0), N - 1) : 0;
                PCS_DCHECK(j >= 0 && cloud + j < G && c + 4 <= Cout, "edgeconv infer U row %lld col %d outside %lld x %d",
                           cloud + j, c, G, Cout);
                ub[u] = *reinterpret_cast<const float4*>(U + (cloud + j) * Cout + c);
            }
#pragma unroll
            for (int u = 0; u < EI_FB; ++u) {
                if (k0 + u >= k) break;                // the batch's tail slots read row 0 of the cloud, unused
                mx[0] = fmaxf(mx[0], ub[u].x);
                mx[1] = fmaxf(mx[1], ub[u].y);
                mx[2] = fmaxf(mx[2], ub[u].z);
                mx[3] = fmaxf(mx[3], ub[u].w);
            }
        }
        const float4 o = make_float4(act_f(mx[0] + vi.x, ACT_LRELU, slope), act_f(mx[1] + vi.y, ACT_LRELU, slope),
                                     act_f(mx[2] + vi.z, ACT_LRELU, slope), act_f(mx[3] + vi.w, ACT_LRELU, slope));
        *reinterpret_cast<float4*>(out + g * Cout + c) = o;
        if (out2) *reinterpret_cast<float4*>(out2 + g * ld2 + c) = o;
    }
}

template <int NT>
static void infer_point_launch(int grid, size_t lds, hipStream_t st, const float* X, int ldx, int C, int M,
                               const float* W, int Cout, const float* gamma, const float* beta, const float* rm,
                               const float* rv, float eps, float* U, float* V) {
    // up to 133 KB of the CU's 160 KB of LDS (Cout = C = 128): above the 64 KB default cap
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&edgeconv_infer_point_kernel<NT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)infer_lds_bytes(NT, 128, 16 * NT));
    (void)attr;
    hipLaunchKernelGGL(edgeconv_infer_point_kernel<NT>, dim3(grid), dim3(256), lds, st, X, ldx, C, M, W, Cout, gamma,
                       beta, rm, rv, eps, U, V);
}

}  // namespace pcs

using namespace pcs;

// Eval-mode EdgeConv forward.  X (B*N rows, stride ldx) with C channels, idx (B, N, k) int32
// per-cloud neighbour table, W (Cout, 2C) = the Conv2d weight, BN gamma / beta / running stats
// (read only).  U, V: caller-owned (B*N, Cout) scratch (any contents); out (B*N, Cout) the pooled
// activation, out2 (nullable, row stride ld2) its second copy.  Cout <= 128 and C <= 128: the folded
// weight, 2 Cout x C floats, stays in one block's LDS.  Reference: dgcnn.py:24-77 under eval().
PCS_API int pcs_edgeconv_infer(const float* X, int ldx, int C, const int32_t* idx, int B, int N, int k,
                               const float* W, int Cout, const float* gamma, const float* beta,
                               const float* run_mean, const float* run_var, float eps, float slope, float* U,
                               float* V, float* out, float* out2, int ld2, void* stream) {
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    PCS_CHECK_ARG(B >= 1 && N >= 1 && k >= 1 && k <= N && C >= 1 && C <= 128 && (C < 4 || C % 4 == 0) && Cout >= 4 &&
                      Cout % 4 == 0 && Cout <= 128,
                  "pcs_edgeconv_infer: bad sizes B=%d N=%d k=%d (1 <= k <= N) C=%d (< 4 or %% 4 == 0, <= 128) "
                  "Cout=%d (%% 4 == 0, <= 128)", B, N, k, C, Cout);
    PCS_CHECK_ARG(X && idx && W && gamma && beta && run_mean && run_var && U && V && out,
                  "pcs_edgeconv_infer: null pointer");
    PCS_CHECK_ARG(ldx % 4 == 0 && ldx >= C, "pcs_edgeconv_infer: X row stride %d (%% 4 == 0, >= C=%d)", ldx, C);
    PCS_CHECK_ARG(slope >= 0.f, "pcs_edgeconv_infer: slope %g < 0 (the max moves through a non-decreasing activation)",
                  (double)slope);
    PCS_CHECK_ARG(!out2 || (ld2 >= Cout && ld2 % 4 == 0), "pcs_edgeconv_infer: out2 stride %d (%% 4 == 0, >= Cout=%d)",
                  ld2, Cout);
    PCS_CHECK_ARG(al16(X) && (C < 4 || al16(W)) && al16(U) && al16(V) && al16(out) && al16(out2),
                  "pcs_edgeconv_infer: X, W, U, V, out, out2 must be 16-B aligned");
    const long long G = (long long)B * N;
    PCS_CHECK_ARG(G * k < (1ll << 31), "pcs_edgeconv_infer: too many edges");
    hipStream_t st = as_stream(stream);
    const int NT = 2 * Cout <= 64 ? 2 : 2 * Cout <= 128 ? 4 : 8;
    const size_t lds = infer_lds_bytes(NT, C, Cout);
    const int tiles = (int)((G + EI_ROWS - 1) / EI_ROWS);
    const int pgrid = std::min(tiles, kInferPointBlocks);
    {
        // compulsory bytes: X read once, U and V written; flops: the (G x C) . (C x 2 Cout) product
        ProbeScope pr(st, 4.0 * (double)G * C * Cout, 4.0 * (double)G * (C + 2.0 * Cout),
                      "pcs::edgeconv_infer_point_kernel<%d>", NT);
        if (NT == 2)
            infer_point_launch<2>(pgrid, lds, st, X, ldx, C, (int)G, W, Cout, gamma, beta, run_mean, run_var, eps, U, V);
        else if (NT == 4)
            infer_point_launch<4>(pgrid, lds, st, X, ldx, C, (int)G, W, Cout, gamma, beta, run_mean, run_var, eps, U, V);
        else
            infer_point_launch<8>(pgrid, lds, st, X, ldx, C, (int)G, W, Cout, gamma, beta, run_mean, run_var, eps, U, V);
    }
    const long long pb = 4 * (64 / (Cout / 4));
    const long long need = (G + pb - 1) / pb;
    const long long nb = std::min<long long>(kInferGatherBlocks, need);
    const int ggrid = (int)(nb >= 8 ? (nb + 7) / 8 * 8 : nb);       // a multiple of 8: the XCD-aware order
    {
        // compulsory bytes: U, V and idx read once, out (and out2) written; flops: k maxes + add + act
        ProbeScope pr(st, (double)G * Cout * (k + 2.0), 4.0 * (double)G * ((out2 ? 4.0 : 3.0) * Cout + k),
                      "pcs::edgeconv_infer_gather_kernel");
        hipLaunchKernelGGL(edgeconv_infer_gather_kernel, dim3(ggrid), dim3(256), 0, st, U, V, idx, N, k, Cout, G, slope,
                           out, out2, ld2);
    }
    return launch_status("pcs_edgeconv_infer");
}
