// Single-pass fused AdamW on flat fp32 state buffers (master weights + moments +
// grads concatenated across all parameters): one memory-bound kernel per step
// instead of the ~8 multi-tensor passes of a foreach implementation.
//   m = lerp(m, g, 1-b1); v = b2*v + (1-b2)*g^2
//   master = master*(1 - lr*wd) - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// float4-vectorized, grid-stride, ~2048 blocks (guideline 11).
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace {

__global__ void adamw_kernel(float* __restrict__ master, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ g,
                             long n, float lr, float beta1, float beta2, float eps,
                             float wd_factor, float bc1, float inv_bc2) {
    long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    long stride = (long)gridDim.x * blockDim.x * 4;
    for (long i = i0; i + 4 <= n; i += stride) {
        float4v gv = *reinterpret_cast<const float4v*>(g + i);
        float4v mv = *reinterpret_cast<float4v*>(m + i);
        float4v vv = *reinterpret_cast<float4v*>(v + i);
        float4v pw = *reinterpret_cast<float4v*>(master + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mv[e] = mv[e] + (1.0f - beta1) * (gv[e] - mv[e]);
            vv[e] = beta2 * vv[e] + (1.0f - beta2) * gv[e] * gv[e];
            float denom = sqrtf(vv[e]) * inv_bc2 + eps;
            pw[e] = pw[e] * wd_factor - (lr / bc1) * mv[e] / denom;
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
            m[i] = m[i] + (1.0f - beta1) * (ge - m[i]);
            v[i] = beta2 * v[i] + (1.0f - beta2) * ge * ge;
            float denom = sqrtf(v[i]) * inv_bc2 + eps;
            master[i] = master[i] * wd_factor - (lr / bc1) * m[i] / denom;
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
    float bc1 = 1.0f - powf((float)beta1, (float)step);
    float inv_bc2 = 1.0f / sqrtf(1.0f - powf((float)beta2, (float)step));
    float wd_factor = 1.0f - (float)(lr * weight_decay);
    int threads = 256;
    hipLaunchKernelGGL(adamw_kernel, dim3(elementwise_blocks(n / 4, threads, 2048)), dim3(threads), 0,
                       at::cuda::getCurrentCUDAStream(),
                       master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                       g.data_ptr<float>(), n, (float)lr, (float)beta1, (float)beta2,
                       (float)eps, wd_factor, bc1, inv_bc2);
    HIP_CHECK_LAST();
}
