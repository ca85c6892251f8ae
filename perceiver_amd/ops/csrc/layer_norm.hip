// Fused bf16 LayerNorm forward/backward for CDNA4 (the LN half of SURVEY.md §2.3 K6).
// Memory-bound: one wave64 per row, 16-B granule loads, fp32 accumulation,
// cross-lane shfl_xor reductions; saves per-row mean/rstd for the backward.
// Register caching uses compile-time CHUNKS (static indexing — guide §5.4 rule 20);
// the backward computes dx AND the dW/db per-block partials in one fused pass
// (tiled partial slab + the colsum finalize kernel). The forward's granule
// walk and the slab layout live in row_common.h. The residual stream runs
// through the same kernels: the forward can form s = h + x on the way in
// (add_ln_fwd), the backward can add the shortcut's gradient on the way out
// (ln_bwd with ds), each bit-equal to the torch add it replaces.
#include <ATen/cuda/CUDAContext.h>
#include "row_common.h"

namespace {

constexpr int LN_WPB = 4;  // waves (rows in flight) per block

// CHUNKS = ceil(C / 512); lane handles 8 contiguous elems per chunk.
// ADD: the row is the residual sum s = bf16(h + x) (torch's single rounding),
// written out once and normalised from the rounded value, so y/mean/rstd
// equal ln_fwd(s) while the separate add pass and the re-read of s are gone.
template <int CHUNKS, bool ADD>
__global__ void ln_fwd_kernel(const unsigned short* __restrict__ x,
                              const unsigned short* __restrict__ h,
                              const unsigned short* __restrict__ w,
                              const unsigned short* __restrict__ b,
                              unsigned short* __restrict__ s,
                              unsigned short* __restrict__ y,
                              float* __restrict__ mean_out, float* __restrict__ rstd_out,
                              long rows, int C, float eps) {
    long row = (long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    int lane = threadIdx.x % 64;
    if (row >= rows) return;
    const unsigned short* xrow = x + row * C;
    unsigned short* yrow = y + row * C;

    float vals[CHUNKS][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        if constexpr (ADD) {
            int c0 = granule_col(lane, i);
            visit_granule({h + row * C, xrow}, c0, C, [&](int e, float (&v)[2]) {
                float sv = bf2f(f2bf(v[0] + v[1]));
                vals[i][e] = sv;
                sum += sv;
            });
            store_granule_bf16(s + row * C, c0, C, [&](int e) { return vals[i][e]; });
        } else {
            visit_granule({xrow}, granule_col(lane, i), C, [&](int e, float (&v)[1]) {
                vals[i][e] = v[0];
                sum += v[0];
            });
        }
    }
    sum = wave_sum(sum);
    float mean = sum / C;
    // Variance from a centred second pass over the cached row, in range only.
    // sumsq / C - mean * mean cancels mean^2 / var of the fp32 precision, up to
    // 2^16 for bf16 rows that sit on two neighbouring values (docs/kernels.md).
    float ssq = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        int c0 = granule_col(lane, i);
        if (c0 + 8 <= C) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float d = vals[i][e] - mean;
                ssq += d * d;
            }
        } else if (c0 < C) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < C) {
                    float d = vals[i][e] - mean;
                    ssq += d * d;
                }
        }
    }
    float var = wave_sum(ssq) / C;
    float rstd = rsqrtf(var + eps);
    if (lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }

    // weight and bias both arrive as granules; the branch is wave-uniform
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
        int c0 = granule_col(lane, i);
        float o[8];
        if (b)
            visit_granule({w, b}, c0, C, [&](int e, float (&v)[2]) {
                o[e] = (vals[i][e] - mean) * rstd * v[0] + v[1];
            });
        else
            visit_granule({w}, c0, C, [&](int e, float (&v)[1]) {
                float bb = 0.f;
                o[e] = (vals[i][e] - mean) * rstd * v[0] + bb;
            });
        store_granule_bf16(yrow, c0, C, [&](int e) { return o[e]; });
    }
}

// dx (+ ds): the residual gradient joins after dx is rounded to bf16, the
// order of the separate bf16 add this replaces.
template <bool HAS_DS>
DEVINL float add_ds(float dx, unsigned short ds) {
    if constexpr (HAS_DS) return bf2f(f2bf(dx)) + bf2f(ds);
    return dx;
}

// The two backward kernels below each write out their own granule walk and
// row arithmetic instead of calling visit_granule or one shared row function:
// every restructuring tried moved which a*b+c the compiler contracts into
// FMAs, and with it dx by one bf16 ulp in a few elements per million
// (docs/kernels.md). Keep the two row bodies in step by hand.
template <int CHUNKS, bool HAS_DS>
__global__ void ln_bwd_dx_kernel(const unsigned short* __restrict__ dy,
                                 const unsigned short* __restrict__ x,
                                 const unsigned short* __restrict__ w,
                                 const float* __restrict__ mean_in,
                                 const float* __restrict__ rstd_in,
                                 const unsigned short* __restrict__ ds,
                                 unsigned short* __restrict__ dx,
                                 long rows, int C) {
    long row = (long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    int lane = threadIdx.x % 64;
    if (row >= rows) return;
    const unsigned short* dyrow = dy + row * C;
    const unsigned short* xrow = x + row * C;
    unsigned short* dxrow = dx + row * C;
    float mean = mean_in[row], rstd = rstd_in[row];

    const unsigned short* dsrow = HAS_DS ? ds + row * C : nullptr;

    float g[CHUNKS][8], xh[CHUNKS][8];
    short8v dsv[CHUNKS];  // whole ds granules, fetched with dy/x (dead without ds)
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
            if constexpr (HAS_DS) dsv[i] = *reinterpret_cast<const short8v*>(dsrow + c0);
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
                o[e] = (short)f2bf(add_ds<HAS_DS>(rstd * (g[i][e] - s1 - xh[i][e] * s2),
                                                  HAS_DS ? (unsigned short)dsv[i][e] : 0));
            *reinterpret_cast<short8v*>(dxrow + c0) = o;
        } else if (c0 < C) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < C)
                    dxrow[c0 + e] = f2bf(add_ds<HAS_DS>(rstd * (g[i][e] - s1 - xh[i][e] * s2),
                                                        HAS_DS ? dsrow[c0 + e] : 0));
        }
    }
}

// Fused backward: dx AND the dw/db per-block partials in ONE pass over
// dy/x. The separate dwdb kernel re-read the same 2*rows*C bf16 and paid a
// per-row mean/rstd load chain — ~55 us/call on the MLM shapes where the
// dx-only kernel runs the identical traffic in ~21 us. One wave per row,
// grid-stride row loop, per-lane fp32 dw/db accumulators, LDS combine,
// tiled partial slab (slab_index: same layout + finalize as colsum).
//
// The reduction grid leaves only 2-3 waves on a SIMD, too few to cover the
// load latency with one row per wave in flight. PIPE therefore keeps the NEXT
// row's whole granules (and its mean/rstd) in flight, packed as loaded, while
// the current row is reduced and stored: the loads are issued as soon as the
// first pass has unpacked the current row. The row arithmetic inside the two
// arms is untouched, only where a whole granule's bits come from moves.
template <int CHUNKS, bool HAS_DS, bool PIPE>
__launch_bounds__(256, (CHUNKS >= 3 || PIPE) ? 2 : 4)  // wide rows need >128 VGPRs
__global__ void ln_bwd_fused_kernel(const unsigned short* __restrict__ dy,
                                    const unsigned short* __restrict__ x,
                                    const unsigned short* __restrict__ w,
                                    const float* __restrict__ mean_in,
                                    const float* __restrict__ rstd_in,
                                    const unsigned short* __restrict__ ds,
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

    // the row in flight (PIPE): whole granules only, the ragged one is read in place
    short8v dyq[CHUNKS], xq[CHUNKS], dsq[CHUNKS];
    float meanq = 0.f, rstdq = 0.f;
    auto issue = [&](long row) {
        meanq = mean_in[row];
        rstdq = rstd_in[row];
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            int c0 = lane * 8 + i * 512;
            if (c0 + 8 <= C) {
                dyq[i] = *reinterpret_cast<const short8v*>(dy + row * C + c0);
                xq[i] = *reinterpret_cast<const short8v*>(x + row * C + c0);
                if constexpr (HAS_DS) dsq[i] = *reinterpret_cast<const short8v*>(ds + row * C + c0);
            }
        }
    };
    if constexpr (PIPE)
        if (wave0 < rows) issue(wave0);

    for (long row = wave0; row < rows; row += wstride) {
        const unsigned short* dyrow = dy + row * C;
        const unsigned short* xrow = x + row * C;
        const unsigned short* dsrow = HAS_DS ? ds + row * C : nullptr;
        unsigned short* dxrow = dx + row * C;
        float mean, rstd;
        if constexpr (PIPE) { mean = meanq; rstd = rstdq; }
        else { mean = mean_in[row]; rstd = rstd_in[row]; }

        float g[CHUNKS][8], xh[CHUNKS][8];
        short8v dsv[CHUNKS];  // this row's whole ds granules (dead without ds)
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            int c0 = lane * 8 + i * 512;
#pragma unroll
            for (int e = 0; e < 8; ++e) { g[i][e] = 0.f; xh[i][e] = 0.f; }
            if (c0 + 8 <= C) {
                short8v dyv, xv;
                if constexpr (PIPE) {
                    dyv = dyq[i];
                    xv = xq[i];
                    if constexpr (HAS_DS) dsv[i] = dsq[i];
                } else {
                    dyv = *reinterpret_cast<const short8v*>(dyrow + c0);
                    xv = *reinterpret_cast<const short8v*>(xrow + c0);
                    if constexpr (HAS_DS) dsv[i] = *reinterpret_cast<const short8v*>(dsrow + c0);
                }
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
        if constexpr (PIPE)
            if (row + wstride < rows) issue(row + wstride);
        s1 = wave_sum(s1) / C;
        s2 = wave_sum(s2) / C;
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            int c0 = lane * 8 + i * 512;
            if (c0 + 8 <= C) {
                short8v o;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    o[e] = (short)f2bf(add_ds<HAS_DS>(rstd * (g[i][e] - s1 - xh[i][e] * s2),
                                                      HAS_DS ? (unsigned short)dsv[i][e] : 0));
                *reinterpret_cast<short8v*>(dxrow + c0) = o;
            } else if (c0 < C) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (c0 + e < C)
                        dxrow[c0 + e] = f2bf(add_ds<HAS_DS>(rstd * (g[i][e] - s1 - xh[i][e] * s2),
                                                            HAS_DS ? dsrow[c0 + e] : 0));
            }
        }
    }

    // Combine the block's waves (all cover the same column range) and emit one
    // tiled partial row (layout shared with the colsum finalize). Every wave
    // parks its accumulators in a slot of its own with 16-B LDS stores and the
    // block sums the slots in wave order, dw first and db after it through the
    // same slots: a fixed summation order, and none of the 2*C LDS atomics per
    // wave (eight lanes to a bank) that the combine used to cost.
    __shared__ __attribute__((aligned(16))) float red[LN_WPB][CHUNKS * 512];
    const int wv = threadIdx.x / 64;
    auto combine = [&](const float(&acc)[CHUNKS][8], int k) {
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) {
            float* slot = &red[wv][lane * 8 + i * 512];
            *reinterpret_cast<float4v*>(slot) = float4v{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
            *reinterpret_cast<float4v*>(slot + 4) =
                float4v{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float t = red[0][c];
#pragma unroll
            for (int v = 1; v < LN_WPB; ++v) t += red[v][c];
            partial[slab_index(k * C + c, blockIdx.x, gridDim.x)] = t;
        }
    };
    combine(dwacc, 0);
    __syncthreads();  // the slots are read out before db overwrites them
    combine(dbacc, 1);
}

template <int CHUNKS, bool ADD>
void launch_ln_fwd(const torch::Tensor& x, const torch::Tensor* h, const torch::Tensor& w,
                   const c10::optional<torch::Tensor>& b, torch::Tensor* s, torch::Tensor& y,
                   torch::Tensor& mean, torch::Tensor& rstd, long rows, int C, float eps) {
    hipLaunchKernelGGL((ln_fwd_kernel<CHUNKS, ADD>), dim3((rows + LN_WPB - 1) / LN_WPB),
                       dim3(64 * LN_WPB), 0, at::cuda::getCurrentCUDAStream(), bf16_ptr(x),
                       ADD ? bf16_ptr(*h) : nullptr, bf16_ptr(w), opt_bf16_ptr(b),
                       ADD ? bf16_ptr(*s) : nullptr, bf16_ptr(y), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), rows, C, eps);
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
        launch_ln_fwd<decltype(chunks)::value, false>(x, nullptr, wc, b, nullptr, y, mean, rstd,
                                                      rows, C, (float)eps);
    });
    HIP_CHECK_LAST();
    return {y, mean, rstd};
}

// s = h + x (one bf16 rounding, as torch's add) and y = LayerNorm(s) in one
// pass: returns {s, y, mean, rstd}, y/mean/rstd as ln_fwd(s) gives them.
std::vector<torch::Tensor> add_ln_fwd(torch::Tensor h, torch::Tensor x, torch::Tensor w,
                                      c10::optional<torch::Tensor> b, double eps) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(h.is_cuda() && h.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(h.sizes() == x.sizes(), "add_ln_fwd: h and x must have one shape");
    h = h.contiguous();
    x = x.contiguous();
    auto wc = w.contiguous();
    int C = x.size(-1);
    TORCH_CHECK(C <= ROW_MAXC, "add_ln_fwd: C must be <= 2048");
    long rows = x.numel() / C;
    auto s = torch::empty_like(x);
    auto y = torch::empty_like(x);
    auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat32));
    auto rstd = torch::empty_like(mean);
    if (rows == 0) return {s, y, mean, rstd};
    if (has_tensor(b)) b = b->contiguous();
    dispatch_chunks(C, [&](auto chunks) {
        launch_ln_fwd<decltype(chunks)::value, true>(x, &h, wc, b, &s, y, mean, rstd, rows, C,
                                                     (float)eps);
    });
    HIP_CHECK_LAST();
    return {s, y, mean, rstd};
}

// With ds (the gradient arriving on the residual shortcut, shaped like x) the
// first result is bf16(dx) + ds, the sum autograd's fan-in add would form.
std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                  torch::Tensor mean, torch::Tensor rstd, bool needs_dwdb,
                                  c10::optional<torch::Tensor> ds) {
    TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == torch::kBFloat16,
                "ln_bwd: dy must be cuda bf16");
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16, "ln_bwd: x must be cuda bf16");
    TORCH_CHECK(dy.sizes() == x.sizes(), "ln_bwd: dy and x must have one shape");
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16, "ln_bwd: w must be cuda bf16");
    dy = dy.contiguous(); x = x.contiguous();
    auto wc = w.contiguous();
    int C = x.size(-1);
    TORCH_CHECK(C <= ROW_MAXC, "ln_bwd: C must be <= 2048");
    TORCH_CHECK(wc.numel() == C, "ln_bwd: w must hold C elements");
    long rows = x.numel() / C;
    TORCH_CHECK(mean.is_cuda() && mean.scalar_type() == torch::kFloat32 && mean.numel() == rows &&
                rstd.is_cuda() && rstd.scalar_type() == torch::kFloat32 && rstd.numel() == rows,
                "ln_bwd: mean and rstd must be cuda fp32 of one element per row");
    mean = mean.contiguous(); rstd = rstd.contiguous();
    const bool has_ds = has_tensor(ds);
    if (has_ds) {
        TORCH_CHECK(ds->is_cuda() && ds->scalar_type() == torch::kBFloat16 &&
                        ds->sizes() == x.sizes(),
                    "ln_bwd: ds must be cuda bf16 and shaped like x");
        ds = ds->contiguous();
    }
    auto dx = torch::empty_like(x);
    if (rows == 0) return {dx, torch::zeros_like(w), torch::zeros_like(w)};
    // dx only: one row per wave. Otherwise the fused single pass: dx +
    // per-block dw/db partials on the reduction grid + the shared finalize.
    const long nblocks = needs_dwdb ? reduction_blocks(rows, LN_WPB) : (rows + LN_WPB - 1) / LN_WPB;
    // The next-row prefetch pays where its registers cost no wave that the grid
    // would use (measured at 16384x1280, 32768x1024, 65536x768): always
    // without ds; with ds only from three chunks up, where two waves per SIMD
    // are all the reduction grid places anyway. PERCEIVER_LN_BWD_PIPE=0/1
    // forces it off/on for A/B runs.
    static const long pipe_env = env_int("PERCEIVER_LN_BWD_PIPE", -1);
    const bool pipe = pipe_env < 0 ? (!has_ds || C > 1024) : pipe_env != 0;
    torch::Tensor partial;
    if (needs_dwdb) partial = empty_slab(x, 2 * (long)C, nblocks);
    dispatch_chunks(C, [&](auto chunks) {
        constexpr int CHUNKS = decltype(chunks)::value;
        auto stream = at::cuda::getCurrentCUDAStream();
        auto launch = [&](auto kernel, auto... tail) {
            hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(64 * LN_WPB), 0, stream, bf16_ptr(dy),
                               bf16_ptr(x), bf16_ptr(wc), mean.data_ptr<float>(),
                               rstd.data_ptr<float>(), opt_bf16_ptr(ds), bf16_ptr(dx), tail...,
                               rows, C);
        };
        if (!needs_dwdb) {
            if (has_ds) launch(ln_bwd_dx_kernel<CHUNKS, true>);
            else launch(ln_bwd_dx_kernel<CHUNKS, false>);
        } else {
            float* part = partial.data_ptr<float>();
            if (has_ds && pipe) launch(ln_bwd_fused_kernel<CHUNKS, true, true>, part);
            else if (has_ds) launch(ln_bwd_fused_kernel<CHUNKS, true, false>, part);
            else if (pipe) launch(ln_bwd_fused_kernel<CHUNKS, false, true>, part);
            else launch(ln_bwd_fused_kernel<CHUNKS, false, false>, part);
        }
    });
    HIP_CHECK_LAST();
    if (!needs_dwdb) return {dx, torch::Tensor(), torch::Tensor()};
    auto acc = torch::empty({2, (long)C}, x.options());  // bf16 straight out
    colsum_reduce_partials(partial, acc, (int)nblocks, 2 * C);
    return {dx, acc[0], acc[1]};
}

