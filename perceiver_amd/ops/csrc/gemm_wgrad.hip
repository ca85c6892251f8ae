// Split-K weight-gradient GEMM with fused bias-gradient column sums.
//   dy: (M, N) bf16 row-major (upstream gradient)   x: (M, K) bf16 row-major
//   dw[n,k] = sum_m dy[m,n] * x[m,k]   (N, K) bf16
//   db[n]   = sum_m dy[m,n]            (N)    bf16, optional
// fp32 accumulation throughout, one bf16 rounding at the very end.
//
// Why a kernel of its own: the output is small (1280x1280 = 25 tiles of
// 256x256 for 256 CUs) while the reduction is 16384-65536 long, and BOTH
// operands have the reduction index as their slow dimension. The tuned
// library runs this NT shape at ~430 TF/s against ~900-1050 TF/s for the
// forward/dgrad orientations, and the bias gradient then re-reads all of dy.
//   - 256(N) x 256|128(K) output tile, 64 reduction rows per step, 8 waves;
//     the M reduction is split over the grid so tiles x nsplit fills whole
//     rounds of the 256 CUs (wgrad_plan, a pure host function);
//   - both operands are loaded as full row-major lines (16-B loads), written
//     to a 16-column-subtiled LDS image and read back transposed with
//     ds_read_b64_tr_b16 — the recipe the attention backward uses for
//     dV = P^T dO (store_granule / read_frag_tr16 in attn_common.h);
//   - register staging is software-pipelined (issue the loads of step t+2,
//     run the MFMAs of step t, write step t+1 into the other LDS buffer):
//     one barrier per step, HBM latency hidden under the MFMA cluster;
//   - the MFMA takes x as its A operand, so an accumulator's 4 registers are
//     4 consecutive k of one dw row and the fp32 partial tile leaves as 16-B
//     stores;
//   - grid order keeps one split's tiles (same dy/x rows) on one XCD's L2;
//   - workgroups of the first K-tile column add up their dy fragments per
//     lane for db, shared out over the waves that hold the same fragments
//     (uniform branch, compiled out without db);
//   - a second small kernel sums the nsplit fp32 slabs in fixed order and
//     rounds dw and db once. Deterministic, no atomics, no communication
//     between workgroups inside a launch.
#include <ATen/cuda/CUDAContext.h>
#include <tuple>
#include "attn_common.h"

namespace {

constexpr int TN = 256;       // output tile rows (dy columns)
constexpr int BR = 64;        // reduction rows per step (the "K-step")
constexpr int THREADS = 512;  // 8 waves
constexpr int MIN_M = BR;
constexpr int NUM_CU = 256;

constexpr int SUBE = sub16_elems(BR);          // elems per 16-column subtile
constexpr int DY_IMG = (TN / 16) * SUBE * 2;   // bytes

struct WgradPlan {
    int tile_n, tile_k, nsplit;
    long rows_per_split;
};

// Estimated cost (microseconds) of one (tile_k, steps-per-split) choice.
// One round of 256x256x64 tile-steps on all CUs is ~3 us at the ~700 TF/s a
// kernel of this class sustains; the narrower tile does half the flops per
// step at a lower rate. Each split adds one fp32 slab written and read back
// (N*K*8 bytes at ~3 TB/s), and each round a fixed prologue/epilogue.
double plan_cost(long N, long K, int tile_k, long steps_per_split, long nsplit, long rounds) {
    const double step_us = tile_k == 256 ? 3.0 : 1.7;
    const double fixed_us = 3.0;
    const double slab_us = (double)nsplit * (double)N * (double)K * 8.0 / 3.0e6;
    return (double)rounds * ((double)steps_per_split * step_us + fixed_us) + slab_us;
}

int forced_tile_k() {
    static const int forced = (int)env_int("PERCEIVER_WGRAD_TK", 0);
    return forced;
}

}  // namespace

// Pure host planning: output tile and M split for a (M, N, K) weight gradient.
// rows_per_split is a multiple of the K-step; the last split may be shorter,
// none is empty. Among the choices that fill >= 90 % of their last round of
// CUs the cheapest by plan_cost wins (which keeps nsplit, hence slab traffic,
// as small as grid fill allows); if no choice fills that well, the cheapest
// of all. PERCEIVER_WGRAD_TK=128|256 forces a tile for A/B measurement.
static WgradPlan make_wgrad_plan(long M, long N, long K) {
    const long steps = std::max<long>(1, (M + BR - 1) / BR);
    const long tiles_n = std::max<long>(1, (N + TN - 1) / TN);
    WgradPlan best{TN, 128, 1, steps * BR};
    double best_cost = 0;
    bool best_full = false, have = false;
    for (int tile_k : {256, 128}) {
        if (K % tile_k != 0) continue;
        if (forced_tile_k() == 128 && tile_k == 256) continue;
        if (forced_tile_k() == 256 && tile_k == 128 && K % 256 == 0) continue;
        const long tiles = tiles_n * (K / tile_k);
        for (long want = 1; want <= steps; ++want) {
            const long s = (steps + want - 1) / want;  // balanced split length
            const long nsplit = (steps + s - 1) / s;
            if (nsplit != want) continue;  // not reachable without an empty split
            const long blocks = tiles * nsplit;
            const long rounds = (blocks + NUM_CU - 1) / NUM_CU;
            const bool full = blocks * 10 >= rounds * NUM_CU * 9;
            const double cost = plan_cost(N, K, tile_k, s, nsplit, rounds);
            if (!have || (full && !best_full) || (full == best_full && cost < best_cost)) {
                best = WgradPlan{TN, tile_k, (int)nsplit, s * BR};
                best_cost = cost;
                best_full = full;
                have = true;
            }
        }
    }
    return best;
}

std::tuple<int64_t, int64_t, int64_t, int64_t> wgrad_plan(int64_t M, int64_t N, int64_t K) {
    WgradPlan p = make_wgrad_plan(M, N, K);
    return {p.tile_n, p.tile_k, p.nsplit, p.rows_per_split};
}

// Shapes the kernel accepts: N in whole 256-row tiles, K in whole 128-column
// tiles, M in whole K-steps and at least one of them. The fp32 slabs are
// indexed in 32 bits per split. No shape class is turned away for speed:
// against the tuned library's dy^T @ x plus colsum_bf16 the same-machine
// microbenchmark (profiles/r03_wgrad.md) gives 1.7-3.5x on the MLM shapes
// (1280x1280x16384: 0.152 -> 0.092 ms, 256x768x65536: 0.187 -> 0.054 ms),
// 1.9-3.1x on the 512/1536/2048-wide CLM and image classes at 12288 / 55296
// rows, and a tie (0.055 vs 0.053 ms) at the smallest routed shape,
// 256x256x8192.
bool gemm_wgrad_applicable(long M, long N, long K) {
    return N > 0 && K > 0 && N % TN == 0 && K % 128 == 0 && M % BR == 0 && M >= MIN_M &&
           N * K < (1L << 30) && M < (1L << 30);
}

namespace {

template <int TK, bool WANT_DB>
__launch_bounds__(THREADS, 1)
__global__ void gemm_wgrad_kernel(const unsigned short* __restrict__ dyp,  // (M,N)
                                  const unsigned short* __restrict__ xp,   // (M,K)
                                  float* __restrict__ slab,                // (nsplit,N,K)
                                  float* __restrict__ db_part,             // (nsplit,N) or null
                                  int M, int N, int K, int rows_per_split) {
    constexpr int WAVES_K = TK / 64;          // 4 or 2
    constexpr int WAVES_N = 8 / WAVES_K;      // 2 or 4
    constexpr int NEXT = TN / WAVES_N;        // wave extent along n: 128 or 64
    constexpr int NFR = NEXT / 16;            // dy fragments per wave: 8 or 4
    constexpr int KFR = 4;                    // x fragments per wave (64 k)
    constexpr int DB_FR = NFR / WAVES_K;      // dy fragments a wave sums for db: 2
    constexpr int X_IMG = (TK / 16) * SUBE * 2;
    constexpr int BUF = DY_IMG + X_IMG;
    constexpr int NG_DY = TN * BR / 8 / THREADS;  // 16-B granules per thread: 4
    constexpr int NG_X = TK * BR / 8 / THREADS;   // 4 or 2

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int wk = wid % WAVES_K;
    const int wn = wid / WAVES_K;

    // ids run tile-fastest inside a split, so in XCD order the tiles of one
    // split — which read the same dy and x rows — meet in one L2
    const int bid = xcd_block_order(blockIdx.x, gridDim.x);
    const int tiles_k = K / TK;
    const int tiles = (N / TN) * tiles_k;
    const int split = bid / tiles;
    const int tile = bid % tiles;
    const int n0 = (tile / tiles_k) * TN;
    const int k0 = (tile % tiles_k) * TK;
    const int m_begin = split * rows_per_split;
    const int m_end = min(M, m_begin + rows_per_split);
    const int T = (m_end - m_begin) / BR;  // >= 1: the plan leaves no split empty

    float4v acc[KFR][NFR];
#pragma unroll
    for (int i = 0; i < KFR; ++i)
#pragma unroll
        for (int j = 0; j < NFR; ++j) acc[i][j] = float4v{0.f, 0.f, 0.f, 0.f};
    float2v dbacc[DB_FR];
#pragma unroll
    for (int j = 0; j < DB_FR; ++j) dbacc[j] = float2v{0.f, 0.f};
    const bool do_db = WANT_DB && k0 == 0;  // workgroup-uniform

    short8v st_dy[NG_DY], st_x[NG_X];
    auto issue = [&](int t) {
        const long m = (long)m_begin + (long)t * BR;
#pragma unroll
        for (int i = 0; i < NG_DY; ++i) {
            int g = tid + i * THREADS;
            int row = g / (TN / 8), c0 = (g % (TN / 8)) * 8;
            st_dy[i] = *reinterpret_cast<const short8v*>(dyp + (m + row) * N + n0 + c0);
        }
#pragma unroll
        for (int i = 0; i < NG_X; ++i) {
            int g = tid + i * THREADS;
            int row = g / (TK / 8), c0 = (g % (TK / 8)) * 8;
            st_x[i] = *reinterpret_cast<const short8v*>(xp + (m + row) * K + k0 + c0);
        }
    };
    auto write = [&](char* buf) {
#pragma unroll
        for (int i = 0; i < NG_DY; ++i) {
            int g = tid + i * THREADS;
            store_granule<BR, IMG_SUB16>(st_dy[i], g / (TN / 8), (g % (TN / 8)) * 8,
                                         nullptr, 0, buf);
        }
#pragma unroll
        for (int i = 0; i < NG_X; ++i) {
            int g = tid + i * THREADS;
            store_granule<BR, IMG_SUB16>(st_x[i], g / (TK / 8), (g % (TK / 8)) * 8,
                                         nullptr, 0, buf + DY_IMG);
        }
    };

    issue(0);
    write(smem);
    if (T > 1) issue(1);
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const char* dy_img = smem + (t & 1) * BUF;
        const char* x_img = dy_img + DY_IMG;
#pragma unroll
        for (int kk = 0; kk < BR / 32; ++kk) {
            bf16x8 xf[KFR], dyf[NFR];
#pragma unroll
            for (int j = 0; j < NFR; ++j)
                dyf[j] = read_frag_tr16<BR>(dy_img, wn * NFR + j, kk * 32, hi4, lo16);
#pragma unroll
            for (int i = 0; i < KFR; ++i)
                xf[i] = read_frag_tr16<BR>(x_img, wk * KFR + i, kk * 32, hi4, lo16);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < KFR; ++i)
#pragma unroll
                for (int j = 0; j < NFR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[i], dyf[j], acc[i][j],
                                                                        0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            if constexpr (WANT_DB) {
                if (do_db) {
                    // lane holds dy[8 rows][column lo16] of each fragment; the
                    // WAVES_K waves that hold the same fragments share them out
#pragma unroll
                    for (int j = 0; j < NFR; ++j) {
                        if (j / DB_FR != wk) continue;
                        typedef __attribute__((ext_vector_type(4))) unsigned int uint4v;
                        uint4v u;
                        __builtin_memcpy(&u, &dyf[j], 16);
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            dbacc[j % DB_FR] += float2v{__uint_as_float(u[d] << 16),
                                                        __uint_as_float(u[d] & 0xffff0000u)};
                    }
                }
            }
        }
        // the other buffer's readers all passed the previous barrier
        if (t + 1 < T) {
            write(smem + ((t + 1) & 1) * BUF);
            if (t + 2 < T) issue(t + 2);
        }
        __syncthreads();
    }

    // fp32 partial tile: accumulator (i, j) holds dw rows n = 16j + lo16,
    // columns k = 16i + 4*hi4 .. +3
    float* out = slab + (long)split * N * K;
#pragma unroll
    for (int j = 0; j < NFR; ++j) {
        const long n = n0 + wn * NEXT + j * 16 + lo16;
#pragma unroll
        for (int i = 0; i < KFR; ++i) {
            const int k = k0 + wk * 64 + i * 16 + hi4 * 4;
            *reinterpret_cast<float4v*>(out + n * K + k) = acc[i][j];
        }
    }
    if constexpr (WANT_DB) {
        if (do_db) {
#pragma unroll
            for (int j = 0; j < DB_FR; ++j) {
                float s = dbacc[j][0] + dbacc[j][1];
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                if (hi4 == 0)
                    db_part[(long)split * N + n0 + wn * NEXT + (wk * DB_FR + j) * 16 + lo16] = s;
            }
        }
    }
}

// Sums the nsplit fp32 slabs in fixed order and rounds once: blocks below
// dw_blocks each finish 2048 dw elements, the blocks after them finish db.
__launch_bounds__(256)
__global__ void gemm_wgrad_finalize_kernel(const float* __restrict__ slab,
                                           const float* __restrict__ db_part,
                                           unsigned short* __restrict__ dw,
                                           unsigned short* __restrict__ db,
                                           long NK, int N, int nsplit, int dw_blocks) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < dw_blocks) {
        const long e = ((long)blockIdx.x * 256 + tid) * 8;
        if (e >= NK) return;
        float4v a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < nsplit; ++s) {
            const float4v* p = reinterpret_cast<const float4v*>(slab + (long)s * NK + e);
            a += p[0];
            b += p[1];
        }
        short8v o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            o[c] = (short)f2bf(a[c]);
            o[c + 4] = (short)f2bf(b[c]);
        }
        *reinterpret_cast<short8v*>(dw + e) = o;
    } else {
        const int n = ((int)blockIdx.x - dw_blocks) * 256 + tid;
        if (n >= N) return;
        float s = 0.f;
        for (int p = 0; p < nsplit; ++p) s += db_part[(long)p * N + n];
        db[n] = f2bf(s);
    }
}

template <int TK, bool WANT_DB>
void launch_wgrad(const torch::Tensor& dy, const torch::Tensor& x, torch::Tensor& slab,
                  float* db_part, long M, long N, long K, const WgradPlan& p) {
    constexpr size_t smem = 2 * (size_t)(DY_IMG + (TK / 16) * SUBE * 2);
    allow_dynamic_lds<gemm_wgrad_kernel<TK, WANT_DB>>(smem);
    const long grid = (N / TN) * (K / TK) * p.nsplit;
    hipLaunchKernelGGL((gemm_wgrad_kernel<TK, WANT_DB>), dim3(grid), dim3(THREADS), smem,
                       at::cuda::getCurrentCUDAStream(), bf16_ptr(dy), bf16_ptr(x),
                       slab.data_ptr<float>(), db_part, (int)M, (int)N, (int)K,
                       (int)p.rows_per_split);
}

}  // namespace

std::vector<torch::Tensor> gemm_wgrad(torch::Tensor dy, torch::Tensor x, bool want_db) {
    TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == torch::kBFloat16,
                "gemm_wgrad: dy must be cuda bf16");
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16,
                "gemm_wgrad: x must be cuda bf16");
    TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && dy.size(0) == x.size(0),
                "gemm_wgrad: dy (M,N) and x (M,K) must share M");
    dy = dy.contiguous();
    x = x.contiguous();
    const long M = dy.size(0), N = dy.size(1), K = x.size(1);
    TORCH_CHECK(gemm_wgrad_applicable(M, N, K), "gemm_wgrad: unsupported shape ", M, "x", N, "x", K);
    const WgradPlan p = make_wgrad_plan(M, N, K);
    TORCH_CHECK(p.tile_n == TN && K % p.tile_k == 0 && p.nsplit >= 1 &&
                p.rows_per_split % BR == 0 && (long)p.nsplit * p.rows_per_split >= M &&
                (long)(p.nsplit - 1) * p.rows_per_split < M, "gemm_wgrad: bad plan");

    auto f32 = dy.options().dtype(torch::kFloat32);
    auto slab = torch::empty({(long)p.nsplit, N, K}, f32);
    auto dw = torch::empty({N, K}, dy.options());
    torch::Tensor db_part, db;
    float* db_part_p = nullptr;
    unsigned short* db_p = nullptr;
    if (want_db) {
        db_part = torch::empty({(long)p.nsplit, N}, f32);
        db = torch::empty({N}, dy.options());
        db_part_p = db_part.data_ptr<float>();
        db_p = bf16_ptr(db);
    }
    if (p.tile_k == 256) {
        if (want_db) launch_wgrad<256, true>(dy, x, slab, db_part_p, M, N, K, p);
        else launch_wgrad<256, false>(dy, x, slab, db_part_p, M, N, K, p);
    } else {
        if (want_db) launch_wgrad<128, true>(dy, x, slab, db_part_p, M, N, K, p);
        else launch_wgrad<128, false>(dy, x, slab, db_part_p, M, N, K, p);
    }
    HIP_CHECK_LAST();
    const long NK = N * K;
    const int dw_blocks = (int)((NK / 8 + 255) / 256);
    const int db_blocks = want_db ? (int)((N + 255) / 256) : 0;
    hipLaunchKernelGGL(gemm_wgrad_finalize_kernel, dim3(dw_blocks + db_blocks), dim3(256), 0,
                       at::cuda::getCurrentCUDAStream(), slab.data_ptr<float>(), db_part_p,
                       bf16_ptr(dw), db_p, NK, (int)N, p.nsplit, dw_blocks);
    HIP_CHECK_LAST();
    if (want_db) return {dw, db};
    return {dw};
}
