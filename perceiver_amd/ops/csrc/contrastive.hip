// Contrastive search on the captured-graph decode path: the max-cosine sweep of
// a group's k candidate hidden states over its history (contrastive_sim), the
// per-group score / commit / next proposal (contrastive_commit) and the copy of
// the winner's freshly appended KV row over its group (contrastive_copy). All
// three read what changes between requests or steps (history length, alpha, EOS
// and fill ids, the record cursor, cache lengths) from device memory, so one
// captured graph serves every request. Plain vector stores, no atomics, nothing
// crosses workgroups inside a launch; the grids depend on host shapes only.
//
// contrastive_sim, grid (nsplit, G), the memory-bound stream:
//   - the group's k candidate rows are staged once in LDS as bf16 (k * C * 2
//     bytes, padded to K = 2, 4 or 8 slots with zeros);
//   - a history row of C channels is LPR = min(64, pow2ceil(C / 8)) lanes of
//     16-byte chunks (lane t takes chunks t, t + LPR, ...), so one load
//     instruction of a wave covers 64 / LPR rows (the row granule), and four
//     granules are in flight per wave. Rows go straight from global memory to
//     VGPRs; a lane reads its chunk of every candidate from LDS once per four
//     rows;
//   - dot products accumulate in fp32 and are reduced over the LPR lanes by xor
//     butterflies, scaled by the row's reciprocal norm and folded into k running
//     maxima held as order keys: the result does not depend on the order of the
//     sweep, and NaN propagates as in amax;
//   - the group cuts [0, hist_len) into nsplit slices of equal size (rounded up
//     to the granule), so work follows the live length. hist_len is clamped into
//     [0, cap] before any address is formed. A slice without rows writes -inf.
//
// contrastive_commit, one block per group:
//   1. the group's old candidate tokens and probabilities are staged in LDS
//      before anything is written;
//   2. r_j = 1 / max(||h_j||, 1e-12) of the k candidates, block sums through a
//      fixed tree; thread 0 finishes sim_j = (max over the partials) * r_j
//      (0 with an empty history, the one deviation from amax), scores
//      (1 - a) p_j - a sim_j, picks sel (lowest j on ties, NaN largest) and
//      writes the emitted token at the record cursor, done and src;
//   3. row sel's hidden bits and r_sel are appended at hist[min(len, cap - 1)];
//   4. the next k candidates are proposed from row sel's logits: max and
//      sum(exp(x - max)) over the block, then every thread's eight largest
//      (order key, ~index) words in registers and k rounds of "largest word
//      strictly below the previous winner", as beam_select does.
// Without the hidden states it is step 4 alone on row 0 of every group: the
// prefill's proposal.
#include <ATen/cuda/CUDAContext.h>
#include <cstdint>
#include <limits>
#include "common.h"
#include "select_common.h"

namespace {

constexpr int CS_MIN_K = 2;
constexpr int CS_MAX_K = 8;
constexpr int CS_MAXV = 32768;           // decode_select_applicable's range
constexpr int CS_MAX_C = 4088;           // 8 slots of C bf16 + the waves' maxima fill 64 KiB of LDS
constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / WAVE;
constexpr int CS_U = 4;                  // row granules in flight per wave
constexpr long CS_FULL_GRID = 512;       // ~2 workgroups per CU
constexpr long CS_SLICE_ROWS = 64;       // a slice of the capacity keeps at least these rows
constexpr int CS_PART = CS_MAX_K;        // partial maxima per (split, group)
constexpr int CC_BIG_THREADS = 1024;     // commit: vocabularies above CC_SMALL_V
constexpr int CC_SMALL_V = 4096;

typedef __attribute__((ext_vector_type(4))) unsigned int cs_uint4v;

constexpr int cs_pow2ceil(long x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// lanes per history row; the wave's row granule is 64 / cs_lanes_per_row(C)
constexpr int cs_lanes_per_row(long C) {
    const int p = cs_pow2ceil((C + 7) / 8);
    return p > WAVE ? WAVE : p;
}

DEVINL int clamp_len(long long n, int cap) { return n < 0 ? 0 : (n > cap ? cap : (int)n); }

DEVINL void bf8_to_f(short8v v, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bf2f((unsigned short)v[e]);
}

// K candidate slots (k rounded up to 2, 4 or 8), LPR lanes per history row:
// both compile-time, so the butterflies unroll into independent chains
template <int K, int LPR>
__launch_bounds__(CS_THREADS)
__global__ void contrastive_sim_kernel(
    const unsigned short* __restrict__ hp, long h_stride,  // (G * k) rows of C, bf16
    const unsigned short* __restrict__ hist,               // (G, cap, C) bf16
    const float* __restrict__ rnorm,                       // (G, cap)
    const long long* __restrict__ len_p,                   // (1) history length
    float* __restrict__ part,                              // (nsplit, G, CS_PART)
    int k, int cap, int C) {
    // candidates first, then the waves' maxima: the dynamic region starts the
    // LDS allocation, so its base and every 16-byte chunk in it are aligned
    extern __shared__ short8v cs_lds[];
    const int nch = C / 8;
    short8v* cand = cs_lds;  // [K][nch]
    unsigned int* red = reinterpret_cast<unsigned int*>(cs_lds + (long)K * nch);  // [CS_WAVES][K]

    const int split = blockIdx.x, g = blockIdx.y, nsplit = gridDim.x, G = gridDim.y;
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    constexpr int RG = WAVE / LPR;
    const int t = lane % LPR, rg = lane / LPR;

    for (int i = tid; i < K * nch; i += CS_THREADS) {
        const int j = i / nch, c = i - j * nch;
        short8v v = {};
        if (j < k) v = *reinterpret_cast<const short8v*>(hp + ((long)g * k + j) * h_stride + c * 8);
        cand[i] = v;
    }
    __syncthreads();

    const int n = clamp_len(*len_p, cap);
    int per = (n + nsplit - 1) / nsplit;
    per = (per + RG - 1) / RG * RG;
    // begin <= end <= n <= cap: every row in [begin, end) is inside the buffer
    const int begin = min(n, split * per), end = min(n, (split + 1) * per);
    const unsigned short* hrows = hist + (long)g * cap * C;
    const float* rrow = rnorm + (long)g * cap;

    unsigned int best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = 0u;

    // wave-uniform trip count: the butterflies below need every lane
    for (int r0 = begin + wave * (CS_U * RG); r0 < end; r0 += CS_WAVES * CS_U * RG) {
        float acc[CS_U][K];
#pragma unroll
        for (int u = 0; u < CS_U; ++u)
#pragma unroll
            for (int j = 0; j < K; ++j) acc[u][j] = 0.f;
        long row[CS_U];
#pragma unroll
        for (int u = 0; u < CS_U; ++u)  // rows past the slice re-read its last row
            row[u] = min(r0 + u * RG + rg, end - 1);
        for (int c = t; c < nch; c += LPR) {
            float hf[CS_U][8];
#pragma unroll
            for (int u = 0; u < CS_U; ++u)
                bf8_to_f(*reinterpret_cast<const short8v*>(hrows + row[u] * C + c * 8), hf[u]);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                float cf[8];
                bf8_to_f(cand[j * nch + c], cf);
#pragma unroll
                for (int u = 0; u < CS_U; ++u)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[u][j] += cf[e] * hf[u][e];
            }
        }
        // one butterfly stage at a time over all CS_U * K sums: independent chains
#pragma unroll
        for (int x = 1; x < LPR; x <<= 1)
#pragma unroll
            for (int u = 0; u < CS_U; ++u)
#pragma unroll
                for (int j = 0; j < K; ++j) acc[u][j] += __shfl_xor(acc[u][j], x, WAVE);
#pragma unroll
        for (int u = 0; u < CS_U; ++u) {
            const bool valid = r0 + u * RG + rg < end;
            const float r = rrow[row[u]];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const unsigned int key = valid ? order_key(acc[u][j] * r) : 0u;
                best[j] = key > best[j] ? key : best[j];
            }
        }
    }

    // the wave's row groups, then the waves: a maximum, so any order is exact
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int x = LPR; x < WAVE; x <<= 1) {
            const unsigned int o = __shfl_xor(best[j], x, WAVE);
            best[j] = o > best[j] ? o : best[j];
        }
        if (lane == 0) red[wave * K + j] = best[j];
    }
    __syncthreads();
    if (tid < k) {
        unsigned int m = red[tid];
#pragma unroll
        for (int w = 1; w < CS_WAVES; ++w) m = red[w * K + tid] > m ? red[w * K + tid] : m;
        part[((long)split * G + g) * CS_PART + tid] =
            m == 0u ? -std::numeric_limits<float>::infinity() : key_value(m);
    }
}

// Splits aim at CS_FULL_GRID workgroups, at most 32, and a slice of the
// capacity keeps at least CS_SLICE_ROWS rows.
int cs_plan_nsplit(long G, long cap) {
    if (G >= CS_FULL_GRID) return 1;
    const long by_cap = std::max<long>(1, cap / CS_SLICE_ROWS);
    return (int)std::min({(CS_FULL_GRID + G - 1) / G, by_cap, 32L});
}

template <int K, int LPR>
void launch_contrastive_sim_lpr(const unsigned short* h, long h_stride, const unsigned short* hist,
                            const float* rnorm, const long long* len, float* part, int nsplit,
                            int G, int k, int cap, int C) {
    const size_t smem = (size_t)K * C * 2 + (size_t)CS_WAVES * K * sizeof(unsigned int);
    hipLaunchKernelGGL((contrastive_sim_kernel<K, LPR>), dim3(nsplit, G), dim3(CS_THREADS), smem,
                       at::cuda::getCurrentCUDAStream(), h, h_stride, hist, rnorm, len, part, k,
                       cap, C);
    HIP_CHECK_LAST();
}

template <int K>
void launch_contrastive_sim(const unsigned short* h, long h_stride, const unsigned short* hist,
                            const float* rnorm, const long long* len, float* part, int nsplit,
                            int G, int k, int cap, int C) {
    switch (cs_lanes_per_row(C)) {
#define CS_SIM_CASE(LPR_)                                                                        \
    case LPR_:                                                                                   \
        return launch_contrastive_sim_lpr<K, LPR_>(h, h_stride, hist, rnorm, len, part, nsplit, \
                                                   G, k, cap, C);
        CS_SIM_CASE(1) CS_SIM_CASE(2) CS_SIM_CASE(4) CS_SIM_CASE(8) CS_SIM_CASE(16)
        CS_SIM_CASE(32) CS_SIM_CASE(64)
#undef CS_SIM_CASE
    }
    TORCH_CHECK(false, "contrastive_sim: no instantiation for C = ", C);
}

// ---- contrastive_commit ----

struct CommitArgs {
    const void* logits;  // (G * k, V), last dim contiguous
    long logit_stride;   // elements
    int G, k, V;
    long long* tok;      // (G * k) candidate tokens, in and out: what the next step embeds
    float* prob;         // (G * k) candidate probabilities, in and out
    // the commit half; h null: the proposal alone, from row 0 of every group
    const unsigned short* h;  // (G * k) rows of C
    long h_stride;
    const float* part;   // (nsplit, G, CS_PART)
    int nsplit;
    unsigned short* hist;  // (G, cap, C)
    float* rnorm;          // (G, cap)
    const long long* len;  // (1)
    int cap, C;
    unsigned char* done;        // (G) bool, in and out
    int* src;                   // (G * k) out: sel, for the row copy
    const float* alpha;         // (1)
    const long long* eos_fill;  // (2): eos id (< 0: none), fill id
    const long long* step;      // (1) record cursor
    long long* rec;             // (rec_rows, G)
    int rec_rows;
    float* sim_out;    // (G * k) or null
    float* score_out;  // (G * k) or null
};

template <int THREADS>
struct CommitState {
    long long tok[CS_MAX_K];
    float prob[CS_MAX_K], r[CS_MAX_K];
    unsigned long long red[THREADS / WAVE];
    float redf[THREADS / WAVE];
    unsigned long long win[CS_MAX_K];
    int sel;
};

// max / sum over the block, combined in wave order; every thread gets the result
template <int THREADS>
DEVINL unsigned long long cc_block_max(CommitState<THREADS>& st, unsigned long long v) {
    v = wave_max_u64(v);
    __syncthreads();  // the previous result has been read by everyone
    if ((threadIdx.x & (WAVE - 1)) == 0) st.red[threadIdx.x / WAVE] = v;
    __syncthreads();
    unsigned long long r = st.red[0];
#pragma unroll
    for (int w = 1; w < THREADS / WAVE; ++w) r = st.red[w] > r ? st.red[w] : r;
    return r;
}
template <int THREADS>
DEVINL float cc_block_sum(CommitState<THREADS>& st, float v) {
    v = wave_sum_f(v);
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) st.redf[threadIdx.x / WAVE] = v;
    __syncthreads();
    float r = st.redf[0];
#pragma unroll
    for (int w = 1; w < THREADS / WAVE; ++w) r += st.redf[w];
    return r;
}

template <typename T, int THREADS>
__global__ __launch_bounds__(THREADS) void contrastive_commit_kernel(CommitArgs a) {
    __shared__ CommitState<THREADS> st;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int k = a.k, V = a.V;
    const long row0 = (long)g * k;

    // all of the group's old candidates are read before any of them is written
    if (tid < k) {
        st.tok[tid] = a.tok[row0 + tid];
        st.prob[tid] = a.prob[row0 + tid];
    }
    int sel = 0;
    if (a.h) {
        const int nch = a.C / 8;
        for (int j = 0; j < k; ++j) {
            const unsigned short* hrow = a.h + (row0 + j) * a.h_stride;
            float s = 0.f;
            for (int c = tid; c < nch; c += THREADS) {
                float f[8];
                bf8_to_f(*reinterpret_cast<const short8v*>(hrow + c * 8), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += f[e] * f[e];
            }
            s = cc_block_sum(st, s);
            if (tid == 0) st.r[j] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
        }
        const int n = clamp_len(*a.len, a.cap);
        if (tid == 0) {
            const float alpha = *a.alpha;
            const float keep = 1.0f - alpha;
            unsigned long long best = 0ull;
            for (int j = 0; j < k; ++j) {
                unsigned int m = 0u;
                for (int s = 0; s < a.nsplit; ++s) {
                    const unsigned int key = order_key(a.part[((long)s * a.G + g) * CS_PART + j]);
                    m = key > m ? key : m;
                }
                const float sim = n == 0 ? 0.f : __fmul_rn(key_value(m), st.r[j]);
                const float score = __fsub_rn(__fmul_rn(keep, st.prob[j]), __fmul_rn(alpha, sim));
                if (a.sim_out) a.sim_out[row0 + j] = sim;
                if (a.score_out) a.score_out[row0 + j] = score;
                const unsigned long long q = pack_best(order_key(score), j);
                best = q > best ? q : best;
            }
            int s = best_index(best);
            s = s < 0 ? 0 : (s >= k ? k - 1 : s);
            const bool was = a.done[g] != 0;
            const long long emitted = was ? a.eos_fill[1] : st.tok[s];
            a.done[g] = (was || emitted == a.eos_fill[0]) ? 1 : 0;
            const long long cur = a.step ? *a.step : 0ll;
            if (a.rec && cur >= 0 && cur < a.rec_rows) a.rec[cur * a.G + g] = emitted;
            for (int j = 0; j < k; ++j) a.src[row0 + j] = s;
            st.sel = s;
        }
        __syncthreads();
        sel = st.sel;
        // row sel's hidden bits and reciprocal norm join the history
        const int at = n < a.cap ? n : a.cap - 1;
        const unsigned short* hrow = a.h + (row0 + sel) * a.h_stride;
        unsigned short* dst = a.hist + ((long)g * a.cap + at) * a.C;
        for (int c = tid; c < nch; c += THREADS)
            *reinterpret_cast<short8v*>(dst + c * 8) = *reinterpret_cast<const short8v*>(hrow + c * 8);
        if (tid == 0) a.rnorm[(long)g * a.cap + at] = st.r[sel];
    }

    // the next k candidates from row sel's logits
    const T* row = reinterpret_cast<const T*>(a.logits) + (row0 + sel) * a.logit_stride;
    unsigned int km = 0u;
    unsigned long long top[CS_MAX_K] = {};
#pragma unroll 4
    for (int v = tid; v < V; v += THREADS) {
        const unsigned int key = order_key(load_logit(row, v));
        km = key > km ? key : km;
        const unsigned long long q = pack_best(key, v);
        if (q > top[CS_MAX_K - 1]) {
            top[CS_MAX_K - 1] = q;
#pragma unroll
            for (int i = CS_MAX_K - 1; i > 0; --i) {
                const unsigned long long hi = top[i] > top[i - 1] ? top[i] : top[i - 1];
                const unsigned long long lo = top[i] > top[i - 1] ? top[i - 1] : top[i];
                top[i - 1] = hi;
                top[i] = lo;
            }
        }
    }
    const float xmax = key_value((unsigned int)cc_block_max(st, km));
    float sum = 0.f;
#pragma unroll 4
    for (int v = tid; v < V; v += THREADS) sum += expf(load_logit(row, v) - xmax);
    sum = cc_block_sum(st, sum);
    // k rounds of "largest packed word strictly below the previous winner"
    unsigned long long prev = 0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long b = 0ull;
#pragma unroll
        for (int i = 0; i < CS_MAX_K; ++i) {
            const unsigned long long q = top[i];
            b = ((j == 0 || q < prev) && q > b) ? q : b;
        }
        prev = cc_block_max(st, b);
        if (tid == 0) st.win[j] = prev;
    }
    __syncthreads();
    if (tid < k) {
        int v = best_index(st.win[tid]);
        v = v < 0 ? 0 : (v >= V ? V - 1 : v);
        a.tok[row0 + tid] = v;
        a.prob[row0 + tid] = expf(load_logit(row, v) - xmax) / sum;
    }
}

template <typename T>
void launch_contrastive_commit(const CommitArgs& a) {
    auto stream = at::cuda::getCurrentCUDAStream();
    if (a.V <= CC_SMALL_V)
        hipLaunchKernelGGL((contrastive_commit_kernel<T, CS_THREADS>), dim3(a.G), dim3(CS_THREADS),
                           0, stream, a);
    else
        hipLaunchKernelGGL((contrastive_commit_kernel<T, CC_BIG_THREADS>), dim3(a.G),
                           dim3(CC_BIG_THREADS), 0, stream, a);
    HIP_CHECK_LAST();
}

// ---- contrastive_copy ----

constexpr int CP_FIELDS = 6;  // ops/beam.py::reorder_table: base, capacity, units per row, unit bytes, row0, counter index

template <typename U>
DEVINL void copy_row(U* base, long cap, long upr, long r, long first, int k, int s) {
    for (long u = threadIdx.x; u < upr; u += CS_THREADS) {
        const U val = base[((first + s) * cap + r) * upr + u];
        for (int j = 0; j < k; ++j)
            if (j != s) base[((first + j) * cap + r) * upr + u] = val;
    }
}

// grid (buffers, groups): the row at the buffer's length counter, the one this
// step appended, goes from row src[g * k] of the group to the other k - 1
__global__ __launch_bounds__(CS_THREADS) void contrastive_copy_kernel(
    const long long* __restrict__ table, const long long* __restrict__ counters, int ncounters,
    const int* __restrict__ src, int k) {
    const int g = blockIdx.y;
    const long long* d = table + (long)blockIdx.x * CP_FIELDS;
    const long cap = d[1], upr = d[2];
    const long ci = d[5] < 0 ? 0 : (d[5] >= ncounters ? ncounters - 1 : d[5]);
    long r = counters[ci];
    r = r < 0 ? 0 : (r >= cap ? cap - 1 : r);
    int s = src[g * k];
    s = s < 0 ? 0 : (s >= k ? k - 1 : s);
    if (d[3] == 16) copy_row(reinterpret_cast<cs_uint4v*>(d[0]), cap, upr, r, (long)g * k, k, s);
    else copy_row(reinterpret_cast<unsigned short*>(d[0]), cap, upr, r, (long)g * k, k, s);
}

template <typename P>
P* cs_ptr(const torch::Tensor& t, torch::ScalarType st, long n, const torch::Tensor& like,
          const char* name) {
    TORCH_CHECK(t.device() == like.device() && t.scalar_type() == st && t.numel() == n &&
                    t.is_contiguous(),
                "contrastive: ", name, " must be a contiguous tensor of ", n,
                " element(s) of the right dtype on the hiddens' device");
    return reinterpret_cast<P*>(t.data_ptr());
}

// (rows, C) bf16 rows the kernels read with 16-byte loads
void check_hidden_rows(const torch::Tensor& h, long rows, long C, const char* name) {
    TORCH_CHECK(h.is_cuda() && h.scalar_type() == torch::kBFloat16 && h.dim() == 2 &&
                    h.size(0) == rows && h.size(1) == C && h.stride(1) == 1 &&
                    h.stride(0) % 8 == 0 && h.stride(0) >= 0 &&
                    reinterpret_cast<uintptr_t>(h.data_ptr()) % 16 == 0,
                "contrastive: ", name, " must be (", rows, ", ", C,
                ") bf16 on the GPU with 16-byte aligned rows");
}

void check_history(const torch::Tensor& h, const torch::Tensor& hist, const torch::Tensor& rnorm,
                   const torch::Tensor& len, long k) {
    TORCH_CHECK(k >= CS_MIN_K && k <= CS_MAX_K, "contrastive: k out of range");
    TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == torch::kBFloat16 && hist.dim() == 3 &&
                    hist.is_contiguous() && hist.size(0) >= 1 && hist.size(0) <= 65535 &&
                    hist.size(1) >= 1 && hist.size(1) < (1L << 24) &&
                    reinterpret_cast<uintptr_t>(hist.data_ptr()) % 16 == 0,
                "contrastive: hist must be a contiguous (G, cap, C) bf16 tensor on the GPU");
    const long G = hist.size(0), cap = hist.size(1), C = hist.size(2);
    TORCH_CHECK(C >= 8 && C % 8 == 0 && C <= CS_MAX_C, "contrastive: C must be a multiple of 8, at most ", CS_MAX_C);
    check_hidden_rows(h, G * k, C, "h");
    TORCH_CHECK(h.device() == hist.device(), "contrastive: h and hist on different devices");
    cs_ptr<float>(rnorm, torch::kFloat32, G * cap, hist, "rnorm");
    cs_ptr<long long>(len, torch::kInt64, 1, hist, "hist_len");
}

}  // namespace

bool contrastive_applicable(long V, long k, long C) {
    return k >= CS_MIN_K && k <= CS_MAX_K && V >= k && V <= CS_MAXV && C >= 8 && C % 8 == 0 &&
           C <= CS_MAX_C;
}

// host-only: (nsplit, row granule) of contrastive_sim's static grid (nsplit, G)
std::tuple<int64_t, int64_t> contrastive_plan(int64_t G, int64_t cap, int64_t C) {
    TORCH_CHECK(G > 0 && cap > 0 && C > 0, "contrastive_plan: bad arguments");
    return {cs_plan_nsplit(G, cap), WAVE / cs_lanes_per_row(C)};
}

// (nsplit, G, 8) fp32: per slice of [0, hist_len) the k maxima of
// dot(hist_t, h_j) * rnorm_t in slots 0..k-1 (the rest is not written); a slice
// without rows holds -inf
torch::Tensor contrastive_sim(torch::Tensor h, torch::Tensor hist, torch::Tensor rnorm,
                              torch::Tensor hist_len, int64_t k) {
    check_history(h, hist, rnorm, hist_len, k);
    const int G = (int)hist.size(0), cap = (int)hist.size(1), C = (int)hist.size(2);
    const int nsplit = cs_plan_nsplit(G, cap);
    auto part = torch::empty({(long)nsplit, (long)G, (long)CS_PART},
                             hist.options().dtype(torch::kFloat32));
    const long long* len = reinterpret_cast<const long long*>(hist_len.data_ptr<int64_t>());
    if (k <= 2)
        launch_contrastive_sim<2>(bf16_ptr(h), h.stride(0), bf16_ptr(hist), rnorm.data_ptr<float>(),
                                  len, part.data_ptr<float>(), nsplit, G, (int)k, cap, C);
    else if (k <= 4)
        launch_contrastive_sim<4>(bf16_ptr(h), h.stride(0), bf16_ptr(hist), rnorm.data_ptr<float>(),
                                  len, part.data_ptr<float>(), nsplit, G, (int)k, cap, C);
    else
        launch_contrastive_sim<8>(bf16_ptr(h), h.stride(0), bf16_ptr(hist), rnorm.data_ptr<float>(),
                                  len, part.data_ptr<float>(), nsplit, G, (int)k, cap, C);
    return part;
}

// One contrastive step for G groups of k rows. tok and prob hold the group's
// candidates and take the next ones. With h / part / hist / rnorm / hist_len /
// done / src the step commits first (module comment); without them it is the
// proposal alone from row 0 of every group.
void contrastive_commit(torch::Tensor logits, torch::Tensor tok, torch::Tensor prob, int64_t k,
                        c10::optional<torch::Tensor> h, c10::optional<torch::Tensor> part,
                        c10::optional<torch::Tensor> hist, c10::optional<torch::Tensor> rnorm,
                        c10::optional<torch::Tensor> hist_len, c10::optional<torch::Tensor> done,
                        c10::optional<torch::Tensor> src, c10::optional<torch::Tensor> alpha,
                        c10::optional<torch::Tensor> eos_fill, c10::optional<torch::Tensor> step,
                        c10::optional<torch::Tensor> rec, c10::optional<torch::Tensor> sim_out,
                        c10::optional<torch::Tensor> score_out) {
    TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "contrastive_commit: logits must be (B, V) on the GPU");
    TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 || logits.scalar_type() == torch::kFloat32,
                "contrastive_commit: logits must be bf16 or fp32");
    const long B = logits.size(0), V = logits.size(1);
    TORCH_CHECK(k >= CS_MIN_K && k <= CS_MAX_K && V >= k && V <= CS_MAXV,
                "contrastive_commit: V or k out of range (contrastive_applicable)");
    TORCH_CHECK(B > 0 && B % k == 0 && B / k <= 65535 && logits.stride(1) == 1 &&
                    logits.stride(0) >= 0,
                "contrastive_commit: logits must be (G * k, V) with a contiguous vocabulary dim");
    CommitArgs a = {};
    a.logits = logits.data_ptr();
    a.logit_stride = logits.stride(0);
    a.k = (int)k;
    a.G = (int)(B / k);
    a.V = (int)V;
    a.tok = cs_ptr<long long>(tok, torch::kInt64, B, logits, "tok");
    a.prob = cs_ptr<float>(prob, torch::kFloat32, B, logits, "prob");
    if (has_tensor(h)) {
        TORCH_CHECK(has_tensor(part) && has_tensor(hist) && has_tensor(rnorm) &&
                        has_tensor(hist_len) && has_tensor(done) && has_tensor(src) &&
                        has_tensor(alpha) && has_tensor(eos_fill),
                    "contrastive_commit: the commit needs part, hist, rnorm, hist_len, done, src, "
                    "alpha and eos_fill");
        check_history(*h, *hist, *rnorm, *hist_len, k);
        TORCH_CHECK(hist->size(0) == a.G && hist->device() == logits.device(),
                    "contrastive_commit: hist must hold one history per group");
        TORCH_CHECK(part->dim() == 3 && part->size(0) >= 1 && part->size(2) == CS_PART,
                    "contrastive_commit: part must be (nsplit, G, 8)");
        a.h = bf16_ptr(*h);
        a.h_stride = h->stride(0);
        a.nsplit = (int)part->size(0);
        a.part = cs_ptr<const float>(*part, torch::kFloat32, (long)a.nsplit * a.G * CS_PART, logits, "part");
        a.hist = bf16_ptr(*hist);
        a.rnorm = rnorm->data_ptr<float>();
        a.len = reinterpret_cast<const long long*>(hist_len->data_ptr<int64_t>());
        a.cap = (int)hist->size(1);
        a.C = (int)hist->size(2);
        a.done = cs_ptr<unsigned char>(*done, torch::kBool, a.G, logits, "done");
        a.src = cs_ptr<int>(*src, torch::kInt32, B, logits, "src");
        a.alpha = cs_ptr<const float>(*alpha, torch::kFloat32, 1, logits, "alpha");
        a.eos_fill = cs_ptr<const long long>(*eos_fill, torch::kInt64, 2, logits, "eos_fill");
        if (has_tensor(step)) a.step = cs_ptr<const long long>(*step, torch::kInt64, 1, logits, "step");
        if (has_tensor(rec)) {
            TORCH_CHECK(rec->dim() == 2 && rec->size(1) == a.G, "contrastive_commit: rec must be (rows, G)");
            a.rec_rows = (int)rec->size(0);
            a.rec = cs_ptr<long long>(*rec, torch::kInt64, (long)a.rec_rows * a.G, logits, "rec");
        }
        if (has_tensor(sim_out)) a.sim_out = cs_ptr<float>(*sim_out, torch::kFloat32, B, logits, "sim_out");
        if (has_tensor(score_out)) a.score_out = cs_ptr<float>(*score_out, torch::kFloat32, B, logits, "score_out");
    }
    if (logits.scalar_type() == torch::kFloat32) launch_contrastive_commit<float>(a);
    else launch_contrastive_commit<unsigned short>(a);
}

// The row at each buffer's length counter is copied from row src[g * k] of its
// group to the group's other rows, in every buffer of the descriptor table
// (ops/beam.py::reorder_table, which checks the buffers; the start-row column
// is not read).
void contrastive_copy(torch::Tensor table, torch::Tensor counters, torch::Tensor src, int64_t k) {
    TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt64 && table.dim() == 2 &&
                    table.size(1) == CP_FIELDS && table.is_contiguous() && table.size(0) >= 1 &&
                    table.size(0) < 65536,
                "contrastive_copy: table must be a contiguous (nbuf, 6) int64 tensor on the GPU");
    TORCH_CHECK(counters.device() == table.device() && counters.scalar_type() == torch::kInt64 &&
                    counters.is_contiguous() && counters.numel() >= 1,
                "contrastive_copy: counters must be a contiguous int64 tensor on the table's device");
    TORCH_CHECK(k >= CS_MIN_K && k <= CS_MAX_K, "contrastive_copy: k out of range");
    TORCH_CHECK(src.device() == table.device() && src.scalar_type() == torch::kInt32 &&
                    src.is_contiguous() && src.numel() >= k && src.numel() % k == 0 &&
                    src.numel() / k < 65536,
                "contrastive_copy: src must be a contiguous (groups * k) int32 tensor");
    hipLaunchKernelGGL(contrastive_copy_kernel, dim3((int)table.size(0), (int)(src.numel() / k)),
                       dim3(CS_THREADS), 0, at::cuda::getCurrentCUDAStream(),
                       reinterpret_cast<const long long*>(table.data_ptr<int64_t>()),
                       reinterpret_cast<const long long*>(counters.data_ptr<int64_t>()),
                       (int)counters.numel(), src.data_ptr<int>(), (int)k);
    HIP_CHECK_LAST();
}
