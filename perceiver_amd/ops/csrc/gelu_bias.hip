// Fused bias + exact-erf GELU, forward and backward (SURVEY.md §2.3 K6 epilogue
// piece). Memory-bound: bf16 I/O vectorized 8 elements/lane (guideline 13),
// grid-stride loop capped at ~2048 blocks (guideline 11).
//
//   fwd:  y = gelu(x + b)          x: (rows, C) bf16, b: (C) bf16 or absent
//   bwd:  dx = dy * gelu'(x + b)   (db falls out of a matmul-free column sum done
//                                   by the caller on dx_pre when bias is present)
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace {

__global__ void gelu_bias_fwd_kernel_bf16(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ bias,  // may be null
    unsigned short* __restrict__ y,
    long total, int C) {
    long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = i0; i + 8 <= total; i += stride) {
        short8v xv = *reinterpret_cast<const short8v*>(x + i);
        // one modulo per granule: i and C are both multiples of 8, so the
        // 8-element span never wraps the bias row
        const int c0 = bias ? (int)(i % C) : 0;
        short8v yv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = bf2f((unsigned short)xv[j]);
            if (bias) v += bf2f(bias[c0 + j]);
            yv[j] = (short)f2bf(gelu_f(v));
        }
        *reinterpret_cast<short8v*>(y + i) = yv;
    }
}

__global__ void gelu_bias_bwd_kernel_bf16(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ bias,
    const unsigned short* __restrict__ dy,
    unsigned short* __restrict__ dx,
    long total, int C) {
    long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = i0; i + 8 <= total; i += stride) {
        short8v xv = *reinterpret_cast<const short8v*>(x + i);
        short8v gv = *reinterpret_cast<const short8v*>(dy + i);
        const int c0 = bias ? (int)(i % C) : 0;
        short8v ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = bf2f((unsigned short)xv[j]);
            if (bias) v += bf2f(bias[c0 + j]);
            float g = bf2f((unsigned short)gv[j]);
            ov[j] = (short)f2bf(g * gelu_grad_f(v));
        }
        *reinterpret_cast<short8v*>(dx + i) = ov;
    }
}

}  // namespace

// shared host half: dy absent runs the forward, present the backward
static torch::Tensor gelu_bias_run(const torch::Tensor& x, const c10::optional<torch::Tensor>& bias,
                                   const torch::Tensor* dy, const char* name) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && (!dy || dy->is_contiguous()));
    TORCH_CHECK(x.scalar_type() == torch::kBFloat16, name, ": bf16 only");
    auto out = torch::empty_like(x);
    long total = x.numel();
    int C = x.size(-1);
    TORCH_CHECK(C % 8 == 0, "inner dim must be a multiple of 8");
    if (has_tensor(bias)) TORCH_CHECK(bias->is_contiguous() && bias->numel() == C);
    const int threads = 256;
    const dim3 grid(elementwise_blocks(total / 8, threads, 2048));
    auto stream = at::cuda::getCurrentCUDAStream();
    if (dy)
        hipLaunchKernelGGL(gelu_bias_bwd_kernel_bf16, grid, dim3(threads), 0, stream, bf16_ptr(x),
                           opt_bf16_ptr(bias), bf16_ptr(*dy), bf16_ptr(out), total, C);
    else
        hipLaunchKernelGGL(gelu_bias_fwd_kernel_bf16, grid, dim3(threads), 0, stream, bf16_ptr(x),
                           opt_bf16_ptr(bias), bf16_ptr(out), total, C);
    HIP_CHECK_LAST();
    return out;
}

torch::Tensor gelu_bias_fwd(torch::Tensor x, c10::optional<torch::Tensor> bias) {
    return gelu_bias_run(x, bias, nullptr, "gelu_bias_fwd");
}

torch::Tensor gelu_bias_bwd(torch::Tensor x, c10::optional<torch::Tensor> bias, torch::Tensor dy) {
    return gelu_bias_run(x, bias, &dy, "gelu_bias_bwd");
}
