// ITC head / feature-extraction kernels: what follows the projection Linear of
// blip_image_text_matching.py:137-138, 158-159, 260-265 (the Linear itself is a launch of the engine's GEMM).
//   l2_normalize_rows : F.normalize(x, dim=-1) = x / max(||x||_2, eps), eps 1e-12, in place on fp32 rows
//   itc_similarity    : sim[b, t] = sum_e img[b, e] * txt[t, e]   (image_feat @ text_feat.t(), :265)
//   cast_rows         : strided fp32 rows -> contiguous bf16 rows (the bf16 mode's GEMM operand)
// All three are bandwidth / latency trivia next to the encoders (O(rows * E) and O(B * T * E) with E = 256); they are kept
// apart from the GEMM epilogues so that the projection goes through the mode's ordinary dispatch unchanged.
#include "common.h"
#include "kernels.h"

namespace pnp {

// One wave per row (four rows per workgroup): a lane holds E / 64 values in 16-byte pieces (one piece at E = 256), the sum of
// squares is a per-lane fp32 chain in ascending column order followed by the wave's butterfly -- a fixed order, so a row's
// result does not depend on how many rows the launch has.  True division, like torch (x / denom, not x * (1 / denom)).
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(float* __restrict__ x, int rows, int E, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    float* p = x + (size_t)row * E;
    float ss = 0.f;
    for (int c = lane * 4; c < E; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
#pragma unroll
        for (int j = 0; j < 4; j++) ss = fmaf(v[j], v[j], ss);
    }
    ss = wave_sum(ss);
    const float d = fmaxf(sqrtf(ss), eps);
    for (int c = lane * 4; c < E; c += 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = v[j] / d;
        *reinterpret_cast<f32x4*>(p + c) = v;
    }
}

// One thread per (image, text) pair, text index fastest: the lanes of a wave share the image row (one broadcast load) and walk
// 64 text rows.  Plain fp32 FMA, four partial sums over e mod 4 combined as (s0 + s1) + (s2 + s3): the same order for every
// B, T and compute mode.
__global__ __launch_bounds__(256) void itc_similarity_kernel(const float* __restrict__ img, const float* __restrict__ txt,
                                                             float* __restrict__ sim, int B, int T, int E) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * T) return;
    const int b = (int)(idx / T), t = (int)(idx - (long)b * T);
    const float* a = img + (size_t)b * E;
    const float* w = txt + (size_t)t * E;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < E; e += 4) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(a + e);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + e);
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = fmaf(av[j], wv[j], s[j]);
    }
    sim[idx] = (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ __launch_bounds__(256) void cast_rows_kernel(const float* __restrict__ in, int ld_in, bf16* __restrict__ out, int rows,
                                                        int K4) {
    const size_t total = (size_t)rows * K4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / K4;
        const int c = (int)(i - r * K4);
        const f32x4 v = *reinterpret_cast<const f32x4*>(in + r * ld_in + (size_t)c * 4);
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = (bf16)v[j];
        *reinterpret_cast<bf16x4*>(out + (r * K4 + c) * 4) = o;
    }
}

static int ok() { return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP; }

int l2_normalize_rows(float* x, int rows, int E, float eps, hipStream_t s) {
    if (rows <= 0 || E <= 0 || (E & 3)) return PNP_ERR_ARG;
    hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, E, eps);
    return ok();
}

int itc_similarity(const float* img, const float* txt, float* sim, int B, int T, int E, hipStream_t s) {
    if (B <= 0 || T <= 0 || E <= 0 || (E & 3)) return PNP_ERR_ARG;
    const long total = (long)B * T;
    hipLaunchKernelGGL(itc_similarity_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, img, txt, sim, B, T, E);
    return ok();
}

int cast_rows_bf16(const float* in, int ld_in, void* out, int rows, int K, hipStream_t s) {
    if (rows <= 0 || K <= 0 || (K & 3) || (ld_in & 3) || ld_in < K) return PNP_ERR_ARG;
    const size_t total = (size_t)rows * (K / 4);
    const unsigned nb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(cast_rows_kernel, dim3(nb), dim3(256), 0, s, in, ld_in, (bf16*)out, rows, K / 4);
    return ok();
}

}  // namespace pnp
