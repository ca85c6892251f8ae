// Fused bf16 LayerNorm forward/backward for CDNA4 (the LN half of SURVEY.md §2.3 K6).
// Memory-bound: one wave64 per row, 16-B granule loads, fp32 accumulation,
// cross-lane shfl_xor reductions; saves per-row mean/rstd for the backward.
// Register caching uses compile-time CHUNKS (static indexing — guide §5.4 rule 20);
// the backward computes dx AND the dW/db per-block partials in one fused pass
// (tiled partial slab + the colsum finalize kernel). The forward's granule
// walk and the slab layout live in row_common.h.
#include <ATen/cuda/CUDAContext.h>
#include "row_common.h"

namespace {

constexpr int LN_WPB = 4;  // waves (rows in flight) per block

// CHUNKS = ceil(C / 512); lane handles 8 contiguous elems per chunk.
template <int CHUNKS>
__global__ void ln_fwd_kernel(const unsigned short* __restrict__ x,
                              const unsigned short* __restrict__ w,
                              const unsigned short* __restrict__ b,
                              unsigned short* __restrict__ y,
                              float* __restrict__ mean_out, float* __restrict__ rstd_out,
                              long rows, int C, float eps) {
    long row = (long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    int lane = threadIdx.x % 64;
    if (row >= rows) return;
    const unsigned short* xrow = x + row * C;
    unsigned short* yrow = y + row * C;

    float vals[CHUNKS][8];
    float sum = 0.f, sumsq = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i)
        visit_granule({xrow}, granule_col(lane, i), C, [&](int e, float (&v)[1]) {
            vals[i][e] = v[0];
            sum += v[0];
            sumsq += v[0] * v[0];
        });
    sum = wave_sum(sum);
    sumsq = wave_sum(sumsq);
    float mean = sum / C;
    float var = sumsq / C - mean * mean;
    float rstd = rsqrtf(fmaxf(var, 0.f) + eps);
    if (lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }

#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        int c0 = granule_col(lane, i);
        float o[8];
        visit_granule({w}, c0, C, [&](int e, float (&v)[1]) {
            float bb = b ? bf2f(b[c0 + e]) : 0.f;
            o[e] = (vals[i][e] - mean) * rstd * v[0] + bb;
        });
        store_granule_bf16(yrow, c0, C, [&](int e) { return o[e]; });
    }
}

// The two backward kernels below each write out their own granule walk and
// row arithmetic instead of calling visit_granule or one shared row function:
// every restructuring tried moved which a*b+c the compiler contracts into
// FMAs, and with it dx by one bf16 ulp in a few elements per million
// (docs/kernels.md). Keep the two row bodies in step by hand.
template <int CHUNKS>
__global__ void ln_bwd_dx_kernel(const unsigned short* __restrict__ dy,
                                 const unsigned short* __restrict__ x,
                                 const unsigned short* __restrict__ w,
                                 const float* __restrict__ mean_in,
                                 const float* __restrict__ rstd_in,
                                 unsigned short* __restrict__ dx,
                                 long rows, int C) {
    long row = (long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    int lane = threadIdx.x % 64;
    if (row >= rows) return;
    const unsigned short* dyrow = dy + row * C;
    const unsigned short* xrow = x + row * C;
    unsigned short* dxrow = dx + row * C;
    float mean = mean_in[row], rstd = rstd_in[row];

    float g[CHUNKS][8], xh[CHUNKS][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        int c0 = lane * 8 + i * 512;
#pragma unroll
        for (int e = 0; e < 8; ++e) { g[i][e] = 0.f; xh[i][e] = 0.f; }
        if (c0 + 8 <= C) {
            short8v dyv = *reinterpret_cast<const short8v*>(dyrow + c0);
            short8v xv = *reinterpret_cast<const short8v*>(xrow + c0);
            short8v wv = *reinterpret_cast<const short8v*>(w + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float gg = bf2f((unsigned short)dyv[e]) * bf2f((unsigned short)wv[e]);
                float xhat = (bf2f((unsigned short)xv[e]) - mean) * rstd;
                g[i][e] = gg;
                xh[i][e] = xhat;
                s1 += gg;
                s2 += gg * xhat;
            }
        } else if (c0 < C) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (c0 + e < C) {
                    float gg = bf2f(dyrow[c0 + e]) * bf2f(w[c0 + e]);
                    float xhat = (bf2f(xrow[c0 + e]) - mean) * rstd;
                    g[i][e] = gg;
                    xh[i][e] = xhat;
                    s1 += gg;
                    s2 += gg * xhat;
                }
            }
        }
    }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;

#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        int c0 = lane * 8 + i * 512;
        if (c0 + 8 <= C) {
            short8v o;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = (short)f2bf(rstd * (g[i][e] - s1 - xh[i][e] * s2));
            *reinterpret_cast<short8v*>(dxrow + c0) = o;
        } else if (c0 < C) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < C)
                    dxrow[c0 + e] = f2bf(rstd * (g[i][e] - s1 - xh[i][e] * s2));
        }
    }
}

// Fused backward: dx AND the dw/db per-block partials in ONE pass over
// dy/x. The separate dwdb kernel re-read the same 2*rows*C bf16 and paid a
// per-row mean/rstd load chain — ~55 us/call on the MLM shapes where the
// dx-only kernel runs the identical traffic in ~21 us. One wave per row,
// grid-stride row loop, per-lane fp32 dw/db accumulators, LDS combine,
// tiled partial slab (slab_index: same layout + finalize as colsum).
template <int CHUNKS>
__launch_bounds__(256, CHUNKS >= 3 ? 2 : 4)  // wide rows need >128 VGPRs
__global__ void ln_bwd_fused_kernel(const unsigned short* __restrict__ dy,
                                    const unsigned short* __restrict__ x,
                                    const unsigned short* __restrict__ w,
                                    const float* __restrict__ mean_in,
                                    const float* __restrict__ rstd_in,
                                    unsigned short* __restrict__ dx,
                                    float* __restrict__ partial,
                                    long rows, int C) {
    const int lane = threadIdx.x % 64;
    const int wpb = blockDim.x / 64;
    const long wave0 = (long)blockIdx.x * wpb + threadIdx.x / 64;
    const long wstride = (long)gridDim.x * wpb;

    float dwacc[CHUNKS][8], dbacc[CHUNKS][8];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) { dwacc[i][e] = 0.f; dbacc[i][e] = 0.f; }

    for (long row = wave0; row < rows; row += wstride) {
        const unsigned short* dyrow = dy + row * C;
        const unsigned short* xrow = x + row * C;
        unsigned short* dxrow = dx + row * C;
        float mean = mean_in[row], rstd = rstd_in[row];

        float g[CHUNKS][8], xh[CHUNKS][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            int c0 = lane * 8 + i * 512;
#pragma unroll
            for (int e = 0; e < 8; ++e) { g[i][e] = 0.f; xh[i][e] = 0.f; }
            if (c0 + 8 <= C) {
                short8v dyv = *reinterpret_cast<const short8v*>(dyrow + c0);
                short8v xv = *reinterpret_cast<const short8v*>(xrow + c0);
                short8v wv = *reinterpret_cast<const short8v*>(w + c0);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float d = bf2f((unsigned short)dyv[e]);
                    float gg = d * bf2f((unsigned short)wv[e]);
                    float xhat = (bf2f((unsigned short)xv[e]) - mean) * rstd;
                    g[i][e] = gg;
                    xh[i][e] = xhat;
                    s1 += gg;
                    s2 += gg * xhat;
                    dwacc[i][e] += d * xhat;
                    dbacc[i][e] += d;
                }
            } else if (c0 < C) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (c0 + e < C) {
                        float d = bf2f(dyrow[c0 + e]);
                        float gg = d * bf2f(w[c0 + e]);
                        float xhat = (bf2f(xrow[c0 + e]) - mean) * rstd;
                        g[i][e] = gg;
                        xh[i][e] = xhat;
                        s1 += gg;
                        s2 += gg * xhat;
                        dwacc[i][e] += d * xhat;
                        dbacc[i][e] += d;
                    }
                }
            }
        }
        s1 = wave_sum(s1) / C;
        s2 = wave_sum(s2) / C;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            int c0 = lane * 8 + i * 512;
            if (c0 + 8 <= C) {
                short8v o;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    o[e] = (short)f2bf(rstd * (g[i][e] - s1 - xh[i][e] * s2));
                *reinterpret_cast<short8v*>(dxrow + c0) = o;
            } else if (c0 < C) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (c0 + e < C)
                        dxrow[c0 + e] = f2bf(rstd * (g[i][e] - s1 - xh[i][e] * s2));
            }
        }
    }

    // combine the block's waves (all cover the same column range) and emit
    // one tiled partial row (layout shared with the colsum finalize)
    __shared__ float red[2][ROW_MAXC];
    for (int i = threadIdx.x; i < ROW_MAXC; i += blockDim.x) {
        red[0][i] = 0.f;
        red[1][i] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        int c0 = lane * 8 + i * 512;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (c0 + e < C) {
                atomicAdd(&red[0][c0 + e], dwacc[i][e]);  // LDS only
                atomicAdd(&red[1][c0 + e], dbacc[i][e]);
            }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        partial[slab_index(c, blockIdx.x, gridDim.x)] = red[0][c];
        partial[slab_index(C + c, blockIdx.x, gridDim.x)] = red[1][c];
    }
}

}  // namespace

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> b,
                                  double eps) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16);
    x = x.contiguous();
    auto wc = w.contiguous();
    int C = x.size(-1);
    TORCH_CHECK(C <= ROW_MAXC, "ln_fwd: C must be <= 2048");
    long rows = x.numel() / C;
    auto y = torch::empty_like(x);
    auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat32));
    auto rstd = torch::empty_like(mean);
    if (rows == 0) return {y, mean, rstd};
    if (has_tensor(b)) b = b->contiguous();
    dispatch_chunks(C, [&](auto chunks) {
        hipLaunchKernelGGL((ln_fwd_kernel<decltype(chunks)::value>),
                           dim3((rows + LN_WPB - 1) / LN_WPB), dim3(64 * LN_WPB), 0,
                           at::cuda::getCurrentCUDAStream(), bf16_ptr(x), bf16_ptr(wc),
                           opt_bf16_ptr(b), bf16_ptr(y), mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), rows, C, (float)eps);
    });
    HIP_CHECK_LAST();
    return {y, mean, rstd};
}

std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                  torch::Tensor mean, torch::Tensor rstd, bool needs_dwdb) {
    dy = dy.contiguous(); x = x.contiguous();
    auto wc = w.contiguous();
    int C = x.size(-1);
    long rows = x.numel() / C;
    auto dx = torch::empty_like(x);
    if (rows == 0) return {dx, torch::zeros_like(w), torch::zeros_like(w)};
    // dx only: one row per wave. Otherwise the fused single pass: dx +
    // per-block dw/db partials on the reduction grid + the shared finalize.
    const long nblocks = needs_dwdb ? reduction_blocks(rows, LN_WPB) : (rows + LN_WPB - 1) / LN_WPB;
    torch::Tensor partial;
    if (needs_dwdb) partial = empty_slab(x, 2 * (long)C, nblocks);
    dispatch_chunks(C, [&](auto chunks) {
        constexpr int CHUNKS = decltype(chunks)::value;
        auto stream = at::cuda::getCurrentCUDAStream();
        if (needs_dwdb)
            hipLaunchKernelGGL((ln_bwd_fused_kernel<CHUNKS>), dim3(nblocks), dim3(64 * LN_WPB), 0,
                               stream, bf16_ptr(dy), bf16_ptr(x), bf16_ptr(wc),
                               mean.data_ptr<float>(), rstd.data_ptr<float>(), bf16_ptr(dx),
                               partial.data_ptr<float>(), rows, C);
        else
            hipLaunchKernelGGL((ln_bwd_dx_kernel<CHUNKS>), dim3(nblocks), dim3(64 * LN_WPB), 0,
                               stream, bf16_ptr(dy), bf16_ptr(x), bf16_ptr(wc),
                               mean.data_ptr<float>(), rstd.data_ptr<float>(), bf16_ptr(dx),
                               rows, C);
    });
    HIP_CHECK_LAST();
    if (!needs_dwdb) return {dx, torch::Tensor(), torch::Tensor()};
    auto acc = torch::empty({2, (long)C}, x.options());  // bf16 straight out
    colsum_reduce_partials(partial, acc, (int)nblocks, 2 * C);
    return {dx, acc[0], acc[1]};
}
