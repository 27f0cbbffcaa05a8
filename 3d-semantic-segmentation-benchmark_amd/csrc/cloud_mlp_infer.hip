// Eval-mode PointNet stack with a per-cloud max-pool in one pass (reference TNet.forward,
// PointNet.py:23-27, and PointNetEncoder.forward, PointNet.py:80-85, under model.eval()): the
// inference / evaluation path of the stacks whose last layer is wide (1024) and pooled over all N
// points of a cloud.
//
// For cloud b and its rows x_p (p < N, kin channels)
//   a_l    = relu(W'_l a_(l-1) + b'_l)                 l = 1 .. nl - 1      thin layers, widths <= 128
//   out[b] = act( max_p (W'_nl a_(nl-1))_p + b'_nl )   act: ReLU or none    the wide layer
// with eval-mode BatchNorm folded into every conv on the device:
//   s = gamma / sqrt(running_var + eps),  W' = s o W,  b' = s o (bias - running_mean) + beta.
// s is inside W', so the max is over the finished pre-bias activation whatever the sign of gamma
// (gamma == 0: W' = 0, max = 0, out = act(beta) exactly); b' and a ReLU commute with the max
// (x -> fl(x + b') and relu are monotone).  Only per-tile column maxima part[b][tile][c] and the
// (B x C_last) result reach HBM: no (B N x C_last) activation, no pre-BN Z, no BN coefficients.
//
// The thin layers run on the fp32 matrix pipe out of LDS (group_mlp_infer.hip's layer); the wide
// layer on the bf16 pipe with rows_infer.hip's arithmetic, x w ~= hi_x hi_w + hi_x lo_w + lo_x hi_w
// into one fp32 accumulator.  Its left operand, the tile's last thin activation, is split into bf16
// hi / lo planes once, by the thin layer's epilogue, and stays in LDS for every 128-column tile of the
// wide layer; only W' streams.
#include <algorithm>

#include "mlp_common.hpp"

namespace pcs {

constexpr int CMI_ROWS = 128;                    // rows of one cloud per block (32 per wave in the thin layers)
constexpr int CMI_BN = 128;                      // columns of the wide layer per column tile
constexpr int CMI_MAX_THIN = 128;                // thin layer width, and kin
constexpr int CMI_LD = 2 * 32 + 8;               // one LDS row of a 32-K slab: [32 hi | 32 lo | 8 pad] bf16 = 144 B
constexpr int CMI_IMG = 32 * CMI_LD;             // one wave's 32 rows of one slab (bf16 elements)
constexpr int CMI_WSTAGE = CMI_BN * CMI_LD;      // one staged W' slab: 128 columns x 32 K (bf16 elements)
constexpr int CMI_SB = 16;                       // weight loads in flight per thread while staging the thin layers
constexpr size_t CMI_LDS_LIMIT = 160 * 1024;     // one CU's LDS (gfx950)

struct CmiLayer {
    const float *W, *bias, *gamma, *beta, *rm, *rv;
    int ldw, cin, cout;
    float eps;
};

// LDS map.  Region A (from byte 0): per wave `aw` bf16 elements -- first the wave's 32 input rows
// (kin8 + 4 floats each), then, written over them by the last thin layer's epilogue, the split planes of
// its 32 rows of that layer's activation: nslab slab images of 32 rows x 144 B.  Region T (from byte
// tofs): the thin layers' BN scales (128 floats per layer), folded biases (128 per layer), folded weights
// (R = cout rounded to 32 rows of cin8 + 4 floats: the stride = 4 mod 8 keeps the 16 lanes of a
// ds_read_b128 phase on distinct banks) and, with two thin layers, the 128 x (width8 + 4) tile between them.
// The wide layer re-uses region T: two staged W' slabs (2 x 18 KB) and the pool's two 2 x 128 floats.
struct CmiPlan {
    int nthin, kin8, lda, ldm, nslab, ksteps, aw;
    int ldw[2], r32[2], wofs[2], mofs;           // float offsets inside region T
    int tofs;                                    // bytes
    size_t bytes;
};

static inline int cmi_up(int n, int m) { return (n + m - 1) / m * m; }

// The one place the LDS need is computed.  PointNet's stacks: 9|12 -> 64 -> 128 -> 1024 needs 147 KB,
// 64 -> 64 -> 128 -> 1024 (the feature transform's TNet) 159 KB, 64 -> 128 -> 1024 110 KB.
static CmiPlan cmi_plan(int kin, const int* widths, int nl) {
    CmiPlan P{};
    P.nthin = nl - 1;
    P.kin8 = cmi_up(kin, 8);
    P.lda = P.kin8 + 4;
    const int klast = widths[nl - 2];
    P.nslab = cmi_up(klast, 32) / 32;
    P.ksteps = cmi_up(klast, 16) / 16;
    P.aw = std::max(P.nslab * CMI_IMG, 32 * P.lda * 2);
    P.tofs = 4 * P.aw * (int)sizeof(__bf16);
    int off = 2 * CMI_MAX_THIN + 2 * CMI_MAX_THIN, cin = kin;
    for (int l = 0; l < P.nthin; ++l) {
        P.ldw[l] = cmi_up(cin, 8) + 4;
        P.r32[l] = cmi_up(widths[l], 32);
        P.wofs[l] = off;
        off += P.r32[l] * P.ldw[l];
        if (l == 0 && P.nthin == 2) {
            P.ldm = cmi_up(widths[0], 8) + 4;
            P.mofs = off;
            off += CMI_ROWS * P.ldm;
        }
        cin = widths[l];
    }
    const size_t wide = 2 * CMI_WSTAGE * sizeof(__bf16) + 4 * CMI_BN * sizeof(float);
    P.bytes = (size_t)P.tofs + std::max((size_t)off * sizeof(float), wide);
    return P;
}

struct CmiArgs {
    CmiLayer L[3];
    CmiPlan P;
    const float* X;
    float* part;
    int ldx, kin, B, N, tpc, nl, last_relu;      // tpc: tiles per cloud
};

// One thin layer for this wave's 32 rows: acc (32 x 32 NT) = W' . act^T on v_mfma_f32_32x32x2_f32, the
// weight fragment first (lane l32 = the tile's row of either operand, lane half h = channels 8 s + 4 h
// .. + 3, one ds_read_b128 each), so element 4 g + e of tile j is (column 32 j + 8 g + 4 h + e, row l32):
// four consecutive columns of one row per lane.  !SPLIT: b' + ReLU + one float4 into the tile between
// the layers.  SPLIT (the last thin layer): b' + ReLU, then the quad's hi and lo bf16 (8 B each) into
// slab j of the wave's planes; weight rows at or beyond cout are zero with b' = 0, so the K range of
// the wide layer up to the slab's end is written as zeros.  `in` may be the memory `planes` covers: the
// wave's reads of the K loop are all issued before its first write.
template <int NT, bool SPLIT>
__device__ __forceinline__ void cmi_thin(const float* in, int ldi, const float* Wl, const float* bl, int ldw, int cin8,
                                         int cout, float* nxt, int ldn, __bf16* planes, int l32, int h) {
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
#define CMI_MMA(E) \
    _Pragma("unroll") for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j].E, xa.E, acc[j], 0, 0, 0);
        CMI_MMA(x) CMI_MMA(y) CMI_MMA(z) CMI_MMA(w)
#undef CMI_MMA
    }
    const int cout8 = (cout + 7) & ~7;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = 32 * j + 8 * g + 4 * h;
            const float4 b = *reinterpret_cast<const float4*>(bl + n);
            const float v0 = fmaxf(acc[j][4 * g] + b.x, 0.f), v1 = fmaxf(acc[j][4 * g + 1] + b.y, 0.f);
            const float v2 = fmaxf(acc[j][4 * g + 2] + b.z, 0.f), v3 = fmaxf(acc[j][4 * g + 3] + b.w, 0.f);
            if constexpr (!SPLIT) {
                if (n < cout8) *reinterpret_cast<float4*>(nxt + l32 * ldn + n) = make_float4(v0, v1, v2, v3);
            } else {
                const unsigned h0 = bx_pk(v0, v1), h1 = bx_pk(v2, v3);
                // v - float(hi): exact
                const unsigned l0 = bx_pk(v0 - __uint_as_float(h0 << 16), v1 - __uint_as_float(h0 & 0xffff0000u));
                const unsigned l1 = bx_pk(v2 - __uint_as_float(h1 << 16), v3 - __uint_as_float(h1 & 0xffff0000u));
                __bf16* d = planes + j * CMI_IMG + l32 * CMI_LD + 8 * g + 4 * h;
                *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(d + 32) = make_uint2(l0, l1);
            }
        }
}

template <bool SPLIT>
__device__ __forceinline__ void cmi_thin_nt(int nt, const float* in, int ldi, const float* Wl, const float* bl, int ldw,
                                            int cin8, int cout, float* nxt, int ldn, __bf16* planes, int l32, int h) {
    switch (nt) {
    case 1: cmi_thin<1, SPLIT>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, planes, l32, h); break;
    case 2: cmi_thin<2, SPLIT>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, planes, l32, h); break;
    case 3: cmi_thin<3, SPLIT>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, planes, l32, h); break;
    default: cmi_thin<4, SPLIT>(in, ldi, Wl, bl, ldw, cin8, cout, nxt, ldn, planes, l32, h); break;
    }
}

// One block = 4 waves = one tile of 128 rows of ONE cloud (tiles never straddle clouds: tpc =
// ceil(N / 128) per cloud, the last one ragged) and all C_last columns of it.
//
// Thin phase.  The input rows (row p >= N re-reads row N - 1; channels kin .. kin8 are zeros) and the
// thin layers' folded weights go into LDS, then wave w takes rows 32 w .. + 31 through the thin layers;
// the last one leaves the rows' hi / lo planes in region A.
//
// Wide phase.  Steps (column tile ct, slab s), ct outermost, run through one double-buffered pipeline
// that does not drain between column tiles: step i + 1's W' slab (128 columns x 32 K; thread t owns
// units t and t + 256 of 8 consecutive K values, so one thread always stages the same two columns of
// a tile and keeps their BN scale in two registers) is loaded from L2 before step i's MFMAs and
// scaled, split and written into the other stage after them; one barrier per step.  Wave (wm, wn)
// owns rows 64 wm .. + 63 x columns 64 wn .. + 63 of the column tile as 2 x 2 MFMA tiles with the
// ACTIVATION fragment first: accumulator element r of a tile is (row (r & 3) + 8 (r >> 2) + 4 h,
// column l32), so a column's max over the wave's 64 rows is 32 in-lane fmaxf and one __shfl_xor(.., 32).
// After a column tile's last slab the two row halves meet in LDS (the pool buffer alternates with ct:
// a tile's readers and the next tile's writers are one barrier apart), and thread n < 128 adds b',
// applies the ReLU and stores part[b][tile][128 ct + n].  Rows at or beyond N enter the max as -inf.
__global__ __launch_bounds__(256) void cloud_mlp_infer_kernel(const CmiArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cmi_lds[];
    const CmiPlan& P = A.P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.x / A.tpc, tile = blockIdx.x - b * A.tpc;
    const int N = A.N, r0 = tile * CMI_ROWS, nv = min(CMI_ROWS, N - r0);
    __bf16* Ab = reinterpret_cast<__bf16*>(cmi_lds);
    float* T = reinterpret_cast<float*>(cmi_lds + P.tofs);
    float* sscr = T;                                   // BN scales of the thin layers
    float* bthin = T + 2 * CMI_MAX_THIN;               // their folded biases

    // s (the arithmetic of bn_eval_coef_kernel, engine.hip) and b'; rows at or beyond cout are zero
    for (int l = 0; l < P.nthin; ++l) {
        const CmiLayer& L = A.L[l];
        for (int n = tid; n < P.r32[l]; n += 256) {
            float s = 0.f, bb = 0.f;
            if (n < L.cout) {
                s = L.gamma[n] * (1.0f / sqrtf(L.rv[n] + L.eps));
                bb = s * ((L.bias ? L.bias[n] : 0.f) - L.rm[n]) + L.beta[n];
            }
            sscr[CMI_MAX_THIN * l + n] = s;
            bthin[CMI_MAX_THIN * l + n] = bb;
        }
    }
    // the tile's input rows, wave-major: consecutive threads take consecutive quads of a row
    {
        const int nq = P.kin8 / 4;
        for (int e = tid; e < CMI_ROWS * nq; e += 256) {
            const int r = e / nq, c = 4 * (e - r * nq);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < A.kin) {
                const float* xp = A.X + ((size_t)b * N + min(r0 + r, N - 1)) * A.ldx + c;
                PCS_DCHECK_QUAD(xp, A.X, (long long)A.B * N, A.ldx, A.kin, "cloud mlp infer X");
                x = *reinterpret_cast<const float4*>(xp);
                if (c + 1 >= A.kin) x.y = 0.f;
                if (c + 2 >= A.kin) x.z = 0.f;
                if (c + 3 >= A.kin) x.w = 0.f;
            }
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(Ab + (r >> 5) * P.aw) + (r & 31) * P.lda + c) = x;
        }
    }
    __syncthreads();
    // W' = s o W, CMI_SB loads in flight per thread; channels at or beyond cin are zero, every load lies
    // in W's (cout - 1) ldw + cin floats
    for (int l = 0; l < P.nthin; ++l) {
        const CmiLayer& L = A.L[l];
        float* Ws = T + P.wofs[l];
        const float* sv = sscr + CMI_MAX_THIN * l;
        const int ldw = P.ldw[l], total = P.r32[l] * ldw;
        for (int e0 = tid; e0 < total; e0 += CMI_SB * 256) {
            float w[CMI_SB];
#pragma unroll
            for (int u = 0; u < CMI_SB; ++u) {
                const int e = e0 + u * 256, n = e / ldw, c = e - n * ldw;
                const bool in = e < total && n < L.cout && c < L.cin;
                PCS_DCHECK(!in || (size_t)n * L.ldw + c < (size_t)(L.cout - 1) * L.ldw + L.cin,
                           "cloud mlp infer thin W row %d col %d outside %d x %d", n, c, L.cout, L.cin);
                w[u] = in ? L.W[(size_t)n * L.ldw + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < CMI_SB; ++u) {
                const int e = e0 + u * 256;
                if (e < total) Ws[e] = sv[e / ldw] * w[u];
            }
        }
    }
    __syncthreads();

    // ---- thin layers: wave-local rows
    const float* tin = reinterpret_cast<const float*>(Ab + wave * P.aw);
    __bf16* planes = Ab + wave * P.aw;
    if (P.nthin == 1) {
        cmi_thin_nt<true>(P.r32[0] / 32, tin, P.lda, T + P.wofs[0], bthin, P.ldw[0], P.kin8, A.L[0].cout, nullptr, 0,
                          planes, l32, h);
    } else {
        float* mid = T + P.mofs + 32 * wave * P.ldm;
        cmi_thin_nt<false>(P.r32[0] / 32, tin, P.lda, T + P.wofs[0], bthin, P.ldw[0], P.kin8, A.L[0].cout, mid, P.ldm,
                           nullptr, l32, h);
        __syncthreads();
        cmi_thin_nt<true>(P.r32[1] / 32, mid, P.ldm, T + P.wofs[1], bthin + CMI_MAX_THIN, P.ldw[1], P.ldw[1] - 4,
                          A.L[1].cout, nullptr, 0, planes, l32, h);
    }

    // ---- wide layer
    const CmiLayer& L = A.L[A.nl - 1];
    const int cin = L.cin, cout = L.cout, nslab = P.nslab;
    const int nsteps = (cout / CMI_BN) * nslab;
    __bf16* Wd = reinterpret_cast<__bf16*>(cmi_lds + P.tofs);
    float* pool = reinterpret_cast<float*>(Wd + 2 * CMI_WSTAGE);
    const int wm = wave & 1, wn = wave >> 1;
    const int ur[2] = {tid >> 2, 64 + (tid >> 2)}, uk = 8 * (tid & 3);   // units tid, tid + 256: column, K offset
    float4 wa[2], wb[2];
    float sv[2] = {0.f, 0.f};
    auto load_w = [&](int ct, int s) {
        const int k = 32 * s + uk;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int n = ct * CMI_BN + ur[u];               // < cout: cout % 128 == 0
            const float* wp = L.W + (size_t)n * L.ldw + k;
            wa[u] = wb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < cin) {
                PCS_DCHECK_QUAD(wp, L.W, cout, L.ldw, cin, "cloud mlp infer W");
                wa[u] = *reinterpret_cast<const float4*>(wp);
            }
            if (k + 4 < cin) {
                PCS_DCHECK_QUAD(wp + 4, L.W, cout, L.ldw, cin, "cloud mlp infer W");
                wb[u] = *reinterpret_cast<const float4*>(wp + 4);
            }
            if (s == 0) sv[u] = L.gamma[n] * (1.0f / sqrtf(L.rv[n] + L.eps));
        }
    };
    auto store_w = [&](int stage) {
        __bf16* Ws = Wd + stage * CMI_WSTAGE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float s = sv[u];
            uint4 hi, lo;
            bx_split8(make_float4(s * wa[u].x, s * wa[u].y, s * wa[u].z, s * wa[u].w),
                      make_float4(s * wb[u].x, s * wb[u].y, s * wb[u].z, s * wb[u].w), hi, lo);
            *reinterpret_cast<uint4*>(Ws + ur[u] * CMI_LD + uk) = hi;
            *reinterpret_cast<uint4*>(Ws + ur[u] * CMI_LD + uk + 32) = lo;
        }
    };

    load_w(0, 0);                  // in flight while the other waves finish their thin layers
    __syncthreads();               // every wave's planes are written; region T is free
    store_w(0);
    __syncthreads();

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    const __bf16* Xw = Ab + 2 * wm * P.aw + l32 * CMI_LD + 8 * h;
    int ct = 0, s = 0;
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps, last = s == nslab - 1;
        const int ctn = last ? ct + 1 : ct, sn = last ? 0 : s + 1;
        if (more) load_w(ctn, sn);                          // in flight across this step's MFMAs
        const __bf16* Xs = Xw + s * CMI_IMG;
        const __bf16* Ws = Wd + (step & 1) * CMI_WSTAGE + (64 * wn + l32) * CMI_LD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (2 * s + ks >= P.ksteps) break;
            bf16x8 xh[2], xl[2], wh[2], wl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                xh[i] = *reinterpret_cast<const bf16x8*>(Xs + i * P.aw + 16 * ks);
                xl[i] = *reinterpret_cast<const bf16x8*>(Xs + i * P.aw + 16 * ks + 32);
                wh[i] = *reinterpret_cast<const bf16x8*>(Ws + 32 * i * CMI_LD + 16 * ks);
                wl[i] = *reinterpret_cast<const bf16x8*>(Ws + 32 * i * CMI_LD + 16 * ks + 32);
            }
            // the three terms outermost: four independent accumulators between two MFMAs on the same one
#define CMI_MMA(XF, WF)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(XF[i], WF[j], acc[i][j], 0, 0, 0);
            CMI_MMA(xh, wl) CMI_MMA(xl, wh) CMI_MMA(xh, wh)
#undef CMI_MMA
        }
        float* pl = pool + (ct & 1) * 2 * CMI_BN;
        if (last) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float m = -__builtin_inff();
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = 64 * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                        m = fmaxf(m, row < nv ? acc[i][j][r] : -__builtin_inff());
                    }
                    acc[i][j] = f32x16{};
                }
                m = fmaxf(m, __shfl_xor(m, 32, 64));
                if (h == 0) pl[wm * CMI_BN + 64 * wn + 32 * j + l32] = m;
            }
        }
        if (more) store_w((step + 1) & 1);
        __syncthreads();
        if (last && tid < CMI_BN) {
            const int n = ct * CMI_BN + tid;
            const float sc = L.gamma[n] * (1.0f / sqrtf(L.rv[n] + L.eps));
            const float bb = sc * ((L.bias ? L.bias[n] : 0.f) - L.rm[n]) + L.beta[n];
            float y = fmaxf(pl[tid], pl[CMI_BN + tid]) + bb;
            if (A.last_relu) y = fmaxf(y, 0.f);
            const size_t o = ((size_t)b * A.tpc + tile) * cout + n;
            PCS_DCHECK(o < (size_t)A.B * A.tpc * cout, "cloud mlp infer part cloud %d tile %d col %d outside %d x %d x %d", b,
                       tile, n, A.B, A.tpc, cout);
            A.part[o] = y;
        }
        ct = ctn, s = sn;
    }
}

// out[b][c] = max over the cloud's tiles of part[b][tile][c]: fixed order, every element written
__global__ __launch_bounds__(256) void cloud_pool_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                int tpc, int C, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / C;
    const int c = (int)(i - b * C);
    const float* p = part + (size_t)b * tpc * C + c;
    float m = p[0];
    for (int t = 1; t < tpc; ++t) {
        PCS_DCHECK((b * tpc + t) * C + c < total * tpc, "cloud pool reduce cloud %lld tile %d col %d", b, t, c);
        m = fmaxf(m, p[(size_t)t * C]);
    }
    out[i] = m;
}

// Shape checks shared by the two entry points (before any GPU work); fills the layers, widths and kin.
static int cmi_check(const char* who, int B, int N, const pcs_mlp_layer* layers, int nl, CmiArgs& a) {
    PCS_CHECK_ARG(layers, "%s: null pointer", who);
    PCS_CHECK_ARG(nl == 2 || nl == 3, "%s: %d layers (2 or 3)", who, nl);
    PCS_CHECK_ARG(B >= 1 && N >= 1 && (long long)B * N < (1ll << 31), "%s: bad sizes B=%d N=%d", who, B, N);
    int widths[3];
    const long long kin = layers[0].cin;
    PCS_CHECK_ARG(kin >= 4 && kin <= CMI_MAX_THIN, "%s: kin %lld (4 .. %d)", who, kin, CMI_MAX_THIN);
    long long cin = kin;
    for (int l = 0; l < nl; ++l) {
        const pcs_mlp_layer& R = layers[l];
        const bool wide = l == nl - 1;
        PCS_CHECK_ARG(R.W && R.gamma && R.beta && R.run_mean && R.run_var, "%s: layer %d null pointer", who, l);
        PCS_CHECK_ARG(R.use_batch == 0, "%s: layer %d BatchNorm is in training mode", who, l);
        PCS_CHECK_ARG(R.act == ACT_RELU || (wide && R.act == ACT_NONE),
                      "%s: layer %d activation %lld (ReLU; the last layer ReLU or none)", who, l, (long long)R.act);
        PCS_CHECK_ARG(R.cin == cin && R.ldw >= cin && R.ldw < (1ll << 24), "%s: layer %d cin %lld ldw %lld (expected cin %lld)",
                      who, l, (long long)R.cin, (long long)R.ldw, cin);
        if (wide) {
            PCS_CHECK_ARG(R.cout >= CMI_BN && R.cout % CMI_BN == 0 && R.cout <= (1 << 20),
                          "%s: last layer width %lld (a multiple of %d)", who, (long long)R.cout, CMI_BN);
            PCS_CHECK_ARG(R.ldw % 4 == 0 && (reinterpret_cast<uintptr_t>(R.W) & 15) == 0,
                          "%s: last layer W must be 16-B aligned with ldw %% 4 == 0 (ldw %lld)", who, (long long)R.ldw);
        } else {
            PCS_CHECK_ARG(R.cout >= 4 && R.cout % 4 == 0 && R.cout <= CMI_MAX_THIN,
                          "%s: layer %d width %lld (%% 4 == 0, 4 .. %d)", who, l, (long long)R.cout, CMI_MAX_THIN);
        }
        widths[l] = (int)R.cout;
        a.L[l] = CmiLayer{R.W, R.bias, R.gamma, R.beta, R.run_mean, R.run_var, (int)R.ldw, (int)cin, (int)R.cout, (float)R.eps};
        cin = R.cout;
    }
    a.P = cmi_plan((int)kin, widths, nl);
    PCS_CHECK_ARG(a.P.bytes <= CMI_LDS_LIMIT, "%s: the stack needs %zu B of LDS (limit %zu)", who, a.P.bytes, CMI_LDS_LIMIT);
    a.kin = (int)kin, a.B = B, a.N = N, a.nl = nl;
    a.tpc = (N + CMI_ROWS - 1) / CMI_ROWS;
    a.last_relu = layers[nl - 1].act == ACT_RELU;
    PCS_CHECK_ARG((long long)B * a.tpc < (1ll << 31), "%s: too many tiles", who);
    return 0;
}

}  // namespace pcs

using namespace pcs;

// Workspace bytes of pcs_cloud_mlp_infer (the per-tile maxima, B x ceil(N / 128) x C_last floats);
// non-zero (with a message) when the stack is not covered -- the coverage test of the bindings.
PCS_API int pcs_cloud_mlp_infer_workspace(int B, int N, const pcs_mlp_layer* layers, int nl, size_t* bytes) {
    PCS_CHECK_ARG(bytes, "pcs_cloud_mlp_infer_workspace: null pointer");
    CmiArgs a{};
    if (int rc = cmi_check("pcs_cloud_mlp_infer_workspace", B, N, layers, nl, a)) return rc;
    *bytes = (size_t)B * a.tpc * a.L[nl - 1].cout * sizeof(float);
    return 0;
}

// Eval-mode conv + BN (+ ReLU) stack max-pooled over each cloud's N points.  X (B*N rows of kin channels,
// row stride ldx, cloud b = rows b N .. b N + N - 1); layers: nl pcs_mlp_layer records (W .. slope);
// out (B, cout_nl).  Reference: PointNet.py:23-27, 80-85 under eval().
PCS_API int pcs_cloud_mlp_infer(const float* X, int ldx, int kin, int B, int N, const pcs_mlp_layer* layers, int nl,
                                float* out, void* ws, size_t ws_bytes, void* stream) {
    PCS_CHECK_ARG(X && out && ws, "pcs_cloud_mlp_infer: null pointer");
    CmiArgs a{};
    if (int rc = cmi_check("pcs_cloud_mlp_infer", B, N, layers, nl, a)) return rc;
    PCS_CHECK_ARG(kin == a.kin && ldx % 4 == 0 && ldx >= kin && (reinterpret_cast<uintptr_t>(X) & 15) == 0,
                  "pcs_cloud_mlp_infer: kin %d ldx %d (layer 0 cin %d; ldx %% 4 == 0, >= kin; X 16-B aligned)", kin, ldx, a.kin);
    const int C = a.L[nl - 1].cout;
    const size_t need = (size_t)B * a.tpc * C * sizeof(float);
    PCS_CHECK_ARG(ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                  "pcs_cloud_mlp_infer: workspace %zu B (needs %zu)", ws_bytes, need);
    a.X = X, a.ldx = ldx, a.part = static_cast<float*>(ws);
    hipStream_t st = as_stream(stream);
    // up to 160 KB of dynamic LDS: above the 64 KB default cap
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&cloud_mlp_infer_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)CMI_LDS_LIMIT);
    (void)attr;
    double flops = 0.0, wbytes = 0.0;
    for (int l = 0; l < nl; ++l) {
        flops += 2.0 * (double)B * N * a.L[l].cin * a.L[l].cout;
        wbytes += (double)a.L[l].cin * a.L[l].cout;
    }
    {
        // compulsory bytes: X and the weights read once, out written
        ProbeScope pr(st, flops, 4.0 * ((double)B * N * kin + wbytes + (double)B * C), "pcs::cloud_mlp_infer_kernel");
        hipLaunchKernelGGL(cloud_mlp_infer_kernel, dim3(B * a.tpc), dim3(256), a.P.bytes, st, a);
    }
    if (int rc = launch_status("pcs_cloud_mlp_infer")) return rc;
    const long long total = (long long)B * C;
    {
        ProbeScope pr(st, 0.0, (double)need + 4.0 * total, "pcs::cloud_pool_reduce_kernel");
        hipLaunchKernelGGL(cloud_pool_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.part, out,
                           a.tpc, C, total);
    }
    return launch_status("pcs_cloud_mlp_infer");
}
