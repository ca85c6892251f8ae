// Single-pass fused AdamW on flat fp32 state buffers (master weights + moments +
// grads concatenated across all parameters): one memory-bound kernel per step
// instead of the ~8 multi-tensor passes of a foreach implementation.
//   m = lerp(m, g, 1-b1); v = b2*v + (1-b2)*g^2
//   master = master*(1 - lr*wd) - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// The scalar factors (lr/bc1, 1/sqrt(bc2), 1 - lr*wd, 1 - b1, 1 - b2) come from
// the host in double, rounded to fp32 once, as the unfused MasterAdamW path has
// them; the last line is one FMA (error bounds: tests/_pointwise_ref.py).
// float4-vectorized, grid-stride, ~2048 blocks (guideline 11).
#include <ATen/cuda/CUDAContext.h>
#include <cmath>
#include "common.h"

namespace {

__global__ void adamw_kernel(float* __restrict__ master, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ g,
                             long n, float step_size, float one_minus_beta1, float beta2,
                             float one_minus_beta2, float eps, float wd_factor,
                             float inv_bc2) {
    long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    long stride = (long)gridDim.x * blockDim.x * 4;
    for (long i = i0; i + 4 <= n; i += stride) {
        float4v gv = *reinterpret_cast<const float4v*>(g + i);
        float4v mv = *reinterpret_cast<float4v*>(m + i);
        float4v vv = *reinterpret_cast<float4v*>(v + i);
        float4v pw = *reinterpret_cast<float4v*>(master + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mv[e] = mv[e] + one_minus_beta1 * (gv[e] - mv[e]);
            vv[e] = beta2 * vv[e] + one_minus_beta2 * gv[e] * gv[e];
            float denom = sqrtf(vv[e]) * inv_bc2 + eps;
            pw[e] = fmaf(pw[e], wd_factor, -(step_size * mv[e] / denom));
        }
        *reinterpret_cast<float4v*>(m + i) = mv;
        *reinterpret_cast<float4v*>(v + i) = vv;
        *reinterpret_cast<float4v*>(master + i) = pw;
    }
    // scalar tail (block 0)
    long tail = (n / 4) * 4;
    if (blockIdx.x == 0) {
        for (long i = tail + threadIdx.x; i < n; i += blockDim.x) {
            float ge = g[i];
            m[i] = m[i] + one_minus_beta1 * (ge - m[i]);
            v[i] = beta2 * v[i] + one_minus_beta2 * ge * ge;
            float denom = sqrtf(v[i]) * inv_bc2 + eps;
            master[i] = fmaf(master[i], wd_factor, -(step_size * m[i] / denom));
        }
    }
}

}  // namespace

void adamw_step(torch::Tensor master, torch::Tensor m, torch::Tensor v, torch::Tensor g,
                double lr, double beta1, double beta2, double eps, double weight_decay,
                int64_t step) {
    TORCH_CHECK(master.is_cuda() && master.scalar_type() == torch::kFloat32);
    TORCH_CHECK(master.is_contiguous() && m.is_contiguous() && v.is_contiguous() && g.is_contiguous());
    long n = master.numel();
    // every scalar factor in double, rounded to fp32 once: 1 - powf(beta, t) in
    // fp32 put lr/bc1 and 1/sqrt(bc2) up to 2e-5 off the doubles the unfused
    // MasterAdamW path uses, and 1 - (float)beta2 is 1.3e-5 off 1 - beta2
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    const float step_size = (float)(lr / bc1);
    const float inv_bc2 = (float)(1.0 / std::sqrt(bc2));
    const float wd_factor = (float)(1.0 - lr * weight_decay);
    int threads = 256;
    hipLaunchKernelGGL(adamw_kernel, dim3(elementwise_blocks(n / 4, threads, 2048)), dim3(threads), 0,
                       at::cuda::getCurrentCUDAStream(),
                       master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                       g.data_ptr<float>(), n, step_size, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)eps, wd_factor, inv_bc2);
    HIP_CHECK_LAST();
}
