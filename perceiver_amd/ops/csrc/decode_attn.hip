// Single-query attention over per-row key windows for CDNA4 (gfx950): the
// attention of one captured decode step.
//
// out[b, h] = softmax(q[b, h] . k[b, h, lo[b] .. hi[b]]) @ v[b, h, lo[b] .. hi[b]]
//
// q arrives pre-scaled and rotated. lo / hi (both inclusive) are int64 device
// values read by the kernel, so one captured launch serves every window; the
// grid (nsplit, H, B) depends on host shapes only. Both ends are clamped into
// [0, cap) before any address is formed, so no content of lo / hi can cause an
// out-of-range read. A window with hi < lo writes zeros.
//
// The problem is a memory-bound stream of K and V rows (one query row: no MFMA
// tile to fill), so K/V go straight from global memory into VGPRs with 16-byte
// loads, no LDS staging:
//   - a key row of D channels is LPR = pow2ceil(D / 8) lanes of 16 bytes, so one
//     load instruction of a wave covers G = 64 / LPR key rows (the row granule);
//     the lanes of a row hold NV 16-byte chunks of its value row each;
//   - the q fragment lives in registers for the whole sweep; a score is the
//     lane's 8-channel dot product reduced over the LPR lanes by xor butterflies;
//   - online softmax in fp32 (__expf); P stays fp32 (no MFMA, nothing to round);
//   - the G row groups of a wave are combined by xor butterflies, the waves in
//     wave order through LDS.
// Row b cuts ITS window into nsplit slices of equal size (rounded up to G),
// counted from lo[b]: work follows the live length, and every index the
// arithmetic sees is relative to lo[b], so a row's output depends on the
// contents of its window only, not on where the window lies in the buffer.
// Slices past the window's end write an empty partial. decode_attn_merge_kernel
// combines the fp32 partials by logsumexp weights in split order and rounds
// once to bf16: deterministic, no atomics.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <cstdint>
#include "attn_common.h"

namespace {

constexpr int NWAVES = 4;
constexpr float EMPTY_LSE = -1e30f;   // lse of a partial without keys
constexpr long SLICE_KEYS_PER_PARTIAL = 32;  // 32 * nsplit^2 <= cap, see plan_nsplit
constexpr long FULL_GRID = 512;       // ~2 workgroups per CU, as plan_split

constexpr int pow2ceil(long x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// lanes per key row; the wave's row granule is 64 / lanes_per_row(D)
constexpr int lanes_per_row(long D) { return pow2ceil((D + 7) / 8); }

DEVINL int clamp_row(long x, int cap) { return x < 0 ? 0 : (x > cap - 1 ? cap - 1 : (int)x); }

DEVINL float dot8(const float (&q)[8], short8v k) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += q[e] * bf2f((unsigned short)k[e]);
    return s;
}

// LPR lanes per key row, NV value chunks per lane (LPR * NV * 8 >= Dv)
template <int LPR, int NV>
__launch_bounds__(64 * NWAVES)
__global__ void decode_attn_kernel(
    const unsigned short* __restrict__ qp,  // (B,H,1,D) bf16, pre-scaled
    const unsigned short* __restrict__ kp,  // (B,H,cap,D)
    const unsigned short* __restrict__ vp,  // (B,H,cap,Dv)
    const long* __restrict__ lo_p, int lo_stride,  // null: 0; stride 0: one value for all rows
    const long* __restrict__ hi_p, int hi_stride,
    unsigned short* __restrict__ op,        // (B,H,1,Dv), written when gridDim.x == 1
    float* __restrict__ o_part,             // (S,B,H,Dv) fp32, when gridDim.x > 1
    float* __restrict__ lse_part,           // (S,B,H)
    long qsb, long qsh, long ksb, long ksh, long ksn, long vsb, long vsh, long vsn,
    long osb, long osh, int cap, int D, int Dv) {
    constexpr int G = 64 / LPR;
    constexpr int U = NV >= 4 ? 1 : 4 / NV;  // row groups in flight per wave
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int nsplit = gridDim.x, H = gridDim.y, B = gridDim.z;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int t = lane % LPR, g = lane / LPR;

    const long lo_raw = lo_p ? lo_p[(long)b * lo_stride] : 0;
    const long hi_raw = hi_p[(long)b * hi_stride];
    const int lo = clamp_row(lo_raw, cap), hi = clamp_row(hi_raw, cap);
    const int n = hi_raw < lo_raw ? 0 : hi - lo + 1;
    int per = (n + nsplit - 1) / nsplit;
    per = (per + G - 1) / G * G;
    // lo <= begin; end <= hi + 1 <= cap: every row in [begin, end) is in range
    const int end = lo + min(n, (split + 1) * per);
    const int begin = lo + min(n, split * per);

    const int kch = t * 8;
    float qf[8];
    {
        short8v qv = {};
        if (kch < D)
            qv = *reinterpret_cast<const short8v*>(qp + (long)b * qsb + (long)h * qsh + kch);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = bf2f((unsigned short)qv[e]);
    }
    const unsigned short* kbase = kp + (long)b * ksb + (long)h * ksh + kch;
    const unsigned short* vbase = vp + (long)b * vsb + (long)h * vsh + kch;

    float m = EMPTY_LSE, l = 0.f;
    float acc[NV][8];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c][e] = 0.f;

    // wave-uniform trip count: the butterflies below need every lane
    for (int r0 = begin + wave * (U * G); r0 < end; r0 += NWAVES * U * G) {
        short8v kk[U], vv[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // rows past the slice re-read its last row and get weight 0
            const long row = min(r0 + u * G + g, end - 1);
            kk[u] = short8v{};
            if (kch < D) kk[u] = *reinterpret_cast<const short8v*>(kbase + row * ksn);
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                vv[u][c] = short8v{};
                if (kch + c * (LPR * 8) < Dv)
                    vv[u][c] = *reinterpret_cast<const short8v*>(vbase + row * vsn + c * (LPR * 8));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = dot8(qf, kk[u]);
#pragma unroll
            for (int x = 1; x < LPR; x <<= 1) s += __shfl_xor(s, x, 64);
            const bool valid = r0 + u * G + g < end;
            const float m_new = valid ? fmaxf(m, s) : m;
            const float alpha = __expf(m - m_new);
            const float p = valid ? __expf(s - m_new) : 0.f;
            l = l * alpha + p;
#pragma unroll
            for (int c = 0; c < NV; ++c)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    acc[c][e] = acc[c][e] * alpha + p * bf2f((unsigned short)vv[u][c][e]);
            m = m_new;
        }
    }

    // the wave's G row groups
#pragma unroll
    for (int x = LPR; x < 64; x <<= 1) {
        const float m_o = __shfl_xor(m, x, 64), l_o = __shfl_xor(l, x, 64);
        const float m_new = fmaxf(m, m_o);
        const float a = __expf(m - m_new), a_o = __expf(m_o - m_new);
        l = l * a + l_o * a_o;
#pragma unroll
        for (int c = 0; c < NV; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e)
                acc[c][e] = acc[c][e] * a + __shfl_xor(acc[c][e], x, 64) * a_o;
        m = m_new;
    }

    // the workgroup's waves, in wave order
    __shared__ float sm_ml[NWAVES][2];
    __shared__ float sm_acc[NWAVES][NV][LPR][8];
    if (g == 0) {
        if (t == 0) { sm_ml[wave][0] = m; sm_ml[wave][1] = l; }
#pragma unroll
        for (int c = 0; c < NV; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) sm_acc[wave][c][t][e] = acc[c][e];
    }
    __syncthreads();
    if (threadIdx.x >= LPR) return;

    m = sm_ml[0][0];
    l = sm_ml[0][1];
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c][e] = sm_acc[0][c][t][e];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) {
        const float m_o = sm_ml[w][0], l_o = sm_ml[w][1];
        const float m_new = fmaxf(m, m_o);
        const float a = __expf(m - m_new), a_o = __expf(m_o - m_new);
        l = l * a + l_o * a_o;
#pragma unroll
        for (int c = 0; c < NV; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[c][e] = acc[c][e] * a + sm_acc[w][c][t][e] * a_o;
        m = m_new;
    }

    const float inv = l > 0.f ? 1.0f / l : 0.f;  // no keys: zeros
    if (nsplit == 1) {
        unsigned short* orow = op + (long)b * osb + (long)h * osh + kch;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            if (kch + c * (LPR * 8) >= Dv) continue;
            short8v o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(acc[c][e] * inv);
            *reinterpret_cast<short8v*>(orow + c * (LPR * 8)) = o;
        }
        return;
    }
    const long prow = ((long)split * B + b) * H + h;
    float* part = o_part + prow * Dv + kch;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        if (kch + c * (LPR * 8) >= Dv) continue;
#pragma unroll
        for (int e = 0; e < 8; e += 4)
            *reinterpret_cast<float4v*>(part + c * (LPR * 8) + e) =
                float4v{acc[c][e] * inv, acc[c][e + 1] * inv, acc[c][e + 2] * inv,
                        acc[c][e + 3] * inv};
    }
    if (t == 0) lse_part[prow] = l > 0.f ? m + __logf(l) : EMPTY_LSE;
}

// out[b, h, c] = sum_i w_i o_part[i, b, h, c] / sum_i w_i with w_i =
// exp(lse_i - max lse) in split order; empty partials weigh 0, and a row
// whose partials are all empty is zeros. One thread per channel.
__global__ void decode_attn_merge_kernel(const float* __restrict__ o_part,
                                         const float* __restrict__ lse_part,
                                         unsigned short* __restrict__ op, long osb, long osh,
                                         int nsplit, int Dv) {
    const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
    const long rows = (long)gridDim.y * H, row = (long)b * H + h;
    const int c = threadIdx.x;
    if (c >= Dv) return;
    float mx = EMPTY_LSE;
    for (int i = 0; i < nsplit; ++i) mx = fmaxf(mx, lse_part[i * rows + row]);
    float wsum = 0.f, acc = 0.f;
    for (int i = 0; i < nsplit; ++i) {
        const float lse = lse_part[i * rows + row];
        const float w = lse > 0.5f * EMPTY_LSE ? __expf(lse - mx) : 0.f;
        wsum += w;
        acc += w * o_part[(i * rows + row) * Dv + c];
    }
    op[(long)b * osb + (long)h * osh + c] = f2bf(wsum > 0.f ? acc / wsum : 0.f);
}

// Splits aim at FULL_GRID workgroups, at most 32. The merge reads nsplit
// partials per row, so a slice of the capacity keeps at least
// SLICE_KEYS_PER_PARTIAL keys for each of them.
int plan_nsplit(long B, long H, long cap) {
    const long blocks = B * H;
    if (blocks >= FULL_GRID) return 1;
    long by_cap = 1;
    while (SLICE_KEYS_PER_PARTIAL * (by_cap + 1) * (by_cap + 1) <= cap) ++by_cap;
    return (int)std::min({FULL_GRID / blocks + 1, by_cap, 32L});
}

bool aligned16(const torch::Tensor& t) {
    if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) return false;
    for (int d = 0; d < 3; ++d)
        if (t.size(d) > 1 && t.stride(d) % 8) return false;
    return true;
}

template <int LPR, int NV>
void launch_decode_attn(const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
                        const long* lo_p, int lo_stride, const long* hi_p, int hi_stride,
                        torch::Tensor& out, int nsplit) {
    const long B = k.size(0), H = k.size(1), cap = k.size(2), D = k.size(3), Dv = v.size(3);
    auto stream = at::cuda::getCurrentCUDAStream();
    torch::Tensor o_part, lse_part;
    float *o_part_p = nullptr, *lse_part_p = nullptr;
    if (nsplit > 1) {
        auto f32 = q.options().dtype(torch::kFloat32);
        o_part = torch::empty({(long)nsplit, B, H, Dv}, f32);
        lse_part = torch::empty({(long)nsplit, B, H}, f32);
        o_part_p = o_part.data_ptr<float>();
        lse_part_p = lse_part.data_ptr<float>();
    }
    hipLaunchKernelGGL((decode_attn_kernel<LPR, NV>), dim3(nsplit, H, B), dim3(64 * NWAVES), 0,
                       stream, bf16_ptr(q), bf16_ptr(k), bf16_ptr(v), lo_p, lo_stride, hi_p,
                       hi_stride, bf16_ptr(out), o_part_p, lse_part_p,
                       q.size(0) > 1 ? q.stride(0) : 0, q.stride(1),
                       k.stride(0), k.stride(1), k.stride(2),
                       v.stride(0), v.stride(1), v.stride(2),
                       out.stride(0), out.stride(1), (int)cap, (int)D, (int)Dv);
    HIP_CHECK_LAST();
    if (nsplit > 1) {
        hipLaunchKernelGGL(decode_attn_merge_kernel, dim3(H, B), dim3(128), 0, stream,
                           o_part_p, lse_part_p, bf16_ptr(out), out.stride(0), out.stride(1),
                           nsplit, (int)Dv);
        HIP_CHECK_LAST();
    }
}

}  // namespace

bool decode_attn_applicable(long D, long Dv) {
    return D >= 8 && Dv >= 8 && D <= 128 && Dv <= 128 && D % 8 == 0 && Dv % 8 == 0;
}

// host-only: (nsplit, row granule) of the static grid. Depends on shapes alone.
std::tuple<int64_t, int64_t> decode_attn_plan(int64_t B, int64_t H, int64_t cap, int64_t D) {
    TORCH_CHECK(B > 0 && H > 0 && cap > 0 && D > 0 && D <= 128, "decode_attn_plan: bad arguments");
    return {plan_nsplit(B, H, cap), 64 / lanes_per_row(D)};
}

torch::Tensor decode_attn(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                          c10::optional<torch::Tensor> lo, torch::Tensor hi) {
    TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() && hi.is_cuda(), "decode_attn: GPU only");
    TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && k.scalar_type() == torch::kBFloat16 &&
                v.scalar_type() == torch::kBFloat16, "decode_attn: bf16 only");
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4 && q.size(2) == 1,
                "decode_attn: q (B,H,1,D), k (B,H,cap,D), v (B,H,cap,Dv)");
    const long B = k.size(0), H = k.size(1), cap = k.size(2), D = k.size(3), Dv = v.size(3);
    TORCH_CHECK((q.size(0) == B || q.size(0) == 1) && q.size(1) == H && q.size(3) == D &&
                v.size(0) == B && v.size(1) == H && v.size(2) == cap, "decode_attn: shape mismatch");
    TORCH_CHECK(decode_attn_applicable(D, Dv), "decode_attn: unsupported head dims ", D, " ", Dv);
    TORCH_CHECK(B >= 1 && H >= 1 && B <= 65535 && H <= 65535 && cap >= 1 && cap < (1L << 30),
                "decode_attn: sizes out of range");
    TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && v.stride(3) == 1,
                "decode_attn: last dim must be contiguous");
    TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v),
                "decode_attn: rows must be 16-byte aligned");

    auto window_end = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kLong && t.is_contiguous() &&
                    (t.numel() == 1 || t.numel() == B),
                    "decode_attn: ", name, " must be a contiguous int64 GPU tensor of 1 or B elements");
        return t.numel() == 1 ? 0 : 1;
    };
    const long* lo_p = nullptr;
    int lo_stride = 0;
    if (has_tensor(lo)) {
        lo_stride = window_end(*lo, "lo");
        lo_p = reinterpret_cast<const long*>(lo->data_ptr<int64_t>());
    }
    const int hi_stride = window_end(hi, "hi");
    const long* hi_p = reinterpret_cast<const long*>(hi.data_ptr<int64_t>());

    // (B, H, 1, Dv) view of merged-heads (B, 1, H * Dv) memory, as empty_merged_heads
    auto out = torch::empty({B, 1, H, Dv}, q.options()).permute({0, 2, 1, 3});
    const int nsplit = plan_nsplit(B, H, cap);
    const int lpr = lanes_per_row(D);
    const int nv = pow2ceil((Dv / 8 + lpr - 1) / lpr);

#define DECODE_ATTN_CASE(LPR_, NV_)                                                         \
    if (lpr == LPR_ && nv == NV_) {                                                         \
        launch_decode_attn<LPR_, NV_>(q, k, v, lo_p, lo_stride, hi_p, hi_stride, out, nsplit); \
        return out;                                                                         \
    }
    DECODE_ATTN_CASE(16, 1)
    DECODE_ATTN_CASE(8, 1) DECODE_ATTN_CASE(8, 2)
    DECODE_ATTN_CASE(4, 1) DECODE_ATTN_CASE(4, 2) DECODE_ATTN_CASE(4, 4)
    DECODE_ATTN_CASE(2, 1) DECODE_ATTN_CASE(2, 2) DECODE_ATTN_CASE(2, 4) DECODE_ATTN_CASE(2, 8)
    DECODE_ATTN_CASE(1, 1) DECODE_ATTN_CASE(1, 2) DECODE_ATTN_CASE(1, 4) DECODE_ATTN_CASE(1, 8)
    DECODE_ATTN_CASE(1, 16)
#undef DECODE_ATTN_CASE
    TORCH_CHECK(false, "decode_attn: no instantiation for head dims ", D, " ", Dv);
    return out;
}
