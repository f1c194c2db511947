// The stand-alone DenseCRF of include/pnp_hip.h (pnp_crf_create ... pnp_crf_infer): the mean-field of crf_meanfield.hip on unary energies
// the caller brings, with kernel widths the caller chooses, in a solver that owns its workspace and needs no pnp_engine -- what
// pydensecrf's DenseCRF2D is to the reference (PnP_OVSS_0514_updated_segmentation.py:1063-1073).
//
// The workspace, its sizing, the lattice build with its Gaussian-lattice cache, the mean-field sequence and the PostDesc layout
// are crf_solver.h's, shared with the engine's post-processing (post.hip): here one channel group per row and the whole batch
// as one chunk.  This file's own: the solver's argument checks and messages, the compatibility matrices, the KL divergence and
// the two layout kernels between the caller's channel-major (K, H*W) planes (pydensecrf's layout) and the pixel-major Kp-float
// rows the mean-field kernels work on.  The planes <-> rows kernels move floats, and the labels come from the
// last update's own argmax (CrfLabelOut with an identity table).
// Beyond the reference's call (include/pnp_hip.h): per-axis widths (pnp_crf_set_batch_aniso), label-compatibility vectors and
// matrices (pnp_crf_set_compat: crf_update_compat of crf_meanfield.hip takes the update over from crf_update as soon as a term is not
// scalar), stepwise inference (pnp_crf_start / _step / _read; pnp_crf_infer is start + step + emit) and the KL divergence
// (pnp_crf_kl), whose ordered fp64 sums over the per-pixel terms are the only arithmetic of this file.  Gradients of the
// feature-term mean-field: pnp_crf_reserve_grad / pnp_crf_infer_terms_saved / pnp_crf_backward_terms around
// crf_meanfield_backward (crf_solver.h), the cotangent and the unary gradient through the planes <-> rows kernels.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/pnp_hip.h"
#include "common.h"
#include "crf_solver.h"
#include "kernels.h"

using namespace pnp;

namespace pnp {

// ------------------------------------------------------------------------------------------ planes <-> rows
// Both directions of one transpose per image: planes[k][i] (K planes of n = H*W floats, coalesced along the pixels) against
// rows[i][0 .. Kp) (16-byte chunks; floats K .. Kp - 1 are the zero pad crf_update_kernel relies on).  TO_ROWS: ingest of the
// unary energies; otherwise: emit of the marginals.  Plane floats are touched once per call (non-temporal); the rows are what
// the mean-field reads next / has just written.
//
// Narrow rows (Kp < 32): a workgroup parks 256 pixels in an LDS tile [pixel][ldt], as unary_kernel does.  ldt = K + 1 rounded
// up to an ODD number of floats: on the plane side lane l touches float l * ldt + k, and ds_read_b32 / ds_write_b32 bank by
// (address / 4) % 32 within a 32-lane half, so an odd stride visits 32 distinct banks where K + 1 = 22 (21 labels) would put two
// lanes on each of 16.
__host__ __device__ inline int crf_op_ldt(int K) { return (K + 1) | 1; }

template <bool TO_ROWS>
__global__ __launch_bounds__(256) void crf_planes_rows_kernel(const PostDesc* __restrict__ desc, float* __restrict__ planes,
                                                              float* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float ptile[];
    const int b = blockIdx.y;
    const PostDesc d = desc[b];
    const int n = d.H * d.W, K = d.K, ldt = crf_op_ldt(K), R4 = d.Kp >> 2;
    float* const pl = planes + d.off;
    f32x4* const r4 = reinterpret_cast<f32x4*>(rows + d.qoff);
    const int tid = threadIdx.x;
    for (int p0 = blockIdx.x * 256; p0 < n; p0 += gridDim.x * 256) {
        const int np = (n - p0) < 256 ? (n - p0) : 256;
        if (TO_ROWS) {
            if (tid < np) {
                const float* pi = pl + p0 + tid;
                float* row = ptile + tid * ldt;
                int k = 0;
                for (; k + 8 <= K; k += 8) {                             // eight plane loads in flight
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) v[u] = __builtin_nontemporal_load(pi + (size_t)(k + u) * n);
#pragma unroll
                    for (int u = 0; u < 8; u++) row[k + u] = v[u];
                }
                for (; k < K; k++) row[k] = __builtin_nontemporal_load(pi + (size_t)k * n);
            }
            __syncthreads();
            for (int item = tid; item < np * R4; item += 256) {
                const int px = item / R4, c = item - px * R4;
                const float* r = ptile + px * ldt + 4 * c;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = 4 * c + j < K ? r[j] : 0.f;
                r4[(size_t)(p0 + px) * R4 + c] = v;
            }
        } else {
            for (int item = tid; item < np * R4; item += 256) {
                const int px = item / R4, c = item - px * R4;
                const f32x4 v = __builtin_nontemporal_load(r4 + (size_t)(p0 + px) * R4 + c);
                float* r = ptile + px * ldt + 4 * c;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (4 * c + j < K) r[j] = v[j];
            }
            __syncthreads();
            if (tid < np) {
                float* po = pl + p0 + tid;
                const float* row = ptile + tid * ldt;
                for (int k = 0; k < K; k++) __builtin_nontemporal_store(row[k], po + (size_t)k * n);
            }
        }
        __syncthreads();
    }
}

// Wide rows (Kp >= 32): the per-wave form of unary_wide_kernel -- a wave owns 64 pixels and passes 32 floats of their rows at
// a time through its own 64 x 33 tile (8.4 KB per wave whatever K is; stride 33: conflict-free on the plane side), eight
// chunks (128 B) of a row per pass.  No workgroup barrier: a wave's LDS operations execute in order.
template <bool TO_ROWS>
__global__ __launch_bounds__(256) void crf_planes_rows_wide_kernel(const PostDesc* __restrict__ desc, float* __restrict__ planes,
                                                                   float* __restrict__ rows) {
    __shared__ float tiles[4][64][33];
    const int b = blockIdx.y;
    const int n = desc[b].H * desc[b].W, K = desc[b].K, R4 = desc[b].Kp >> 2;
    float* const pl = planes + desc[b].off;
    f32x4* const r4 = reinterpret_cast<f32x4*>(rows + desc[b].qoff);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float (*tile)[33] = tiles[wave];
    for (int p0 = (blockIdx.x * 4 + wave) * 64; p0 < n; p0 += gridDim.x * 256) {
        const bool mine = p0 + lane < n;
        const int i = mine ? p0 + lane : n - 1;                            // lanes past the end redo the last pixel, store nothing
        float* const pi = pl + i;
        for (int cb = 0; cb < R4; cb += 8) {
            const int fb = 4 * cb, kb = fb + 32 < K ? fb + 32 : K;         // channels [fb, kb) fall in this block of the row
            const int ncb = R4 - cb < 8 ? R4 - cb : 8;
            if (TO_ROWS) {
                for (int k = fb; k < kb; k += 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) v[u] = k + u < kb ? __builtin_nontemporal_load(pi + (size_t)(k + u) * n) : 0.f;
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (k + u < kb) tile[lane][k + u - fb] = v[u];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int item = lane; item < 64 * ncb; item += 64) {
                    const int px = item / ncb, c = item - px * ncb;
                    if (p0 + px >= n) continue;
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; j++) v[j] = fb + 4 * c + j < K ? tile[px][4 * c + j] : 0.f;
                    r4[(size_t)(p0 + px) * R4 + cb + c] = v;
                }
            } else {
                for (int item = lane; item < 64 * ncb; item += 64) {
                    const int px = item / ncb, c = item - px * ncb;
                    if (p0 + px >= n) continue;
                    const f32x4 v = __builtin_nontemporal_load(r4 + (size_t)(p0 + px) * R4 + cb + c);
#pragma unroll
                    for (int j = 0; j < 4; j++) tile[px][4 * c + j] = v[j];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (mine)
                    for (int k = fb; k < kb; k++) __builtin_nontemporal_store(tile[lane][k - fb], pi + (size_t)k * n);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// to_rows: planes -> rows (the planes are only read); else rows -> planes (the rows are only read)
static int crf_planes_rows(bool to_rows, const PostDesc* desc, float* planes, float* rows, int B, int maxHW, int max_kp, hipStream_t s) {
    const int tiles = (maxHW + 255) / 256;
    if (max_kp >= 32) {                                                    // (the dispatch of unary_from_maps)
        const dim3 grid(tiles < 2048 ? tiles : 2048, B);
        if (to_rows) hipLaunchKernelGGL(crf_planes_rows_wide_kernel<true>, grid, dim3(256), 0, s, desc, planes, rows);
        else hipLaunchKernelGGL(crf_planes_rows_wide_kernel<false>, grid, dim3(256), 0, s, desc, planes, rows);
    } else {
        const dim3 grid(tiles < 256 ? tiles : 256, B);
        const size_t smem = (size_t)256 * crf_op_ldt(max_kp) * sizeof(float);      // <= 30 KB: K <= max_kp <= 28
        if (to_rows) hipLaunchKernelGGL(crf_planes_rows_kernel<true>, grid, dim3(256), smem, s, desc, planes, rows);
        else hipLaunchKernelGGL(crf_planes_rows_kernel<false>, grid, dim3(256), smem, s, desc, planes, rows);
    }
    return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP;
}

// ------------------------------------------------------------------------------------------ KL divergence: the two-stage sum
// kl_pix holds one fp64 term per pixel (crf_update_compat_kernel<true>).  Stage 1: one partial per run of 256 consecutive
// pixels of an image, added in pixel order by one thread; stage 2: one thread per image adds its partials in order.  The
// order is a function of the image alone, never of the grid.  Partials of image b start at pix0 / 256 + b (>= the runs of the
// images before it).
constexpr int CRF_KL_RUN = 256;
__global__ __launch_bounds__(CRF_KL_RUN) void crf_kl_partial_kernel(const PostDesc* __restrict__ desc, const double* __restrict__ kl_pix,
                                                                   double* __restrict__ part) {
    __shared__ double sh[CRF_KL_RUN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = desc[b].H * desc[b].W, pix0 = desc[b].pix0;
    for (int r = blockIdx.x; r * CRF_KL_RUN < n; r += gridDim.x) {
        const int i = r * CRF_KL_RUN + tid;
        sh[tid] = i < n ? kl_pix[(size_t)pix0 + i] : 0.0;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int j = 0; j < CRF_KL_RUN; j++) s += sh[j];
            part[pix0 / CRF_KL_RUN + b + r] = s;
        }
        __syncthreads();
    }
}
__global__ void crf_kl_final_kernel(const PostDesc* __restrict__ desc, const double* __restrict__ part, double* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int runs = (desc[b].H * desc[b].W + CRF_KL_RUN - 1) / CRF_KL_RUN;
    const double* p = part + desc[b].pix0 / CRF_KL_RUN + b;
    double s = 0.0;
    for (int r = 0; r < runs; r++) s += p[r];
    out[b] = s;
}

// pnp_crf_probe_filter: the value rows of a lattice (Kp floats per point at voff[which] of every image) without their pad, K
// floats per point in id order, image after image
__global__ __launch_bounds__(256) void crf_probe_rows_kernel(const int* __restrict__ idbase, const PostDesc* __restrict__ desc, int which,
                                                             const float* __restrict__ val, float* __restrict__ out) {
    const int b = blockIdx.y;
    size_t base = 0;
    for (int i = 0; i < b; i++) base += (size_t)(idbase[i + 1] - idbase[i]) * desc[i].K;
    const int K = desc[b].K, Kp = desc[b].Kp;
    const size_t n = (size_t)(idbase[b + 1] - idbase[b]) * K;
    const float* const v = val + desc[b].voff[which];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t p = i / K;
        out[base + i] = v[p * Kp + (i - p * K)];
    }
}

}  // namespace pnp

// ------------------------------------------------------------------------------------------ the solver
struct pnp_crf {
    int device = 0;
    // -- fixed by pnp_crf_create
    int maxB = 0, maxK = 0, maxKp = 0, max_pix_img = 0;
    int64_t max_total_pix = 0;
    CrfWorkspace ws;                              // sized for the whole batch as one chunk, one channel group per row
    PostDesc* d_desc = nullptr;
    int32_t* d_lut = nullptr;                     // 0 .. 255: the label of a channel is its index
    size_t* d_label_off = nullptr;                // [B] first pixel of every image in the concatenated label output
    std::vector<void*> allocs;
    size_t alloc_bytes = 0;
    // -- the batch of the last pnp_crf_set_batch
    bool ready = false;
    int B = 0, kp_max = 0, maxHW = 0;
    std::vector<PostDesc> desc;
    std::vector<size_t> h_label_off;              // [B + 1] as d_label_off; [B]: the pixels of the batch
    // -- label compatibility of the two terms (pnp_crf_set_compat; holds until changed).  d_M: two matrices, TRANSPOSED as
    // crf_update_compat reads them (d_M[k * ldm + l] = M[l][k]), row stride ldm = maxKp rounded up to a multiple of 8, zero
    // padded.  A term left scalar is Potts: it takes its weight from the call, and has a matrix (w * I) on the device only
    // while the other term has one or the KL divergence is asked for -- m_scalar_w is the weight that matrix holds
    int kind[2] = {PNP_CRF_COMPAT_SCALAR, PNP_CRF_COMPAT_SCALAR};
    int compat_K[2] = {0, 0};
    int ldm = 0;
    float* d_M = nullptr;
    std::vector<float> h_M;                       // staging of one matrix
    bool m_scalar[2] = {false, false};
    float m_scalar_w[2] = {0.f, 0.f};
    // -- stepwise inference: Q holds the marginals of the last start / step / infer on this batch
    bool started = false;
    double *kl_pix = nullptr, *kl_part = nullptr, *kl_out = nullptr;
    // -- feature terms (pnp_crf_create_terms; max_terms = 0: a two-term solver).  terms_batch: the batch of the last set_batch is
    // one of pnp_crf_set_batch_terms, with T terms of tdims[t] feature axes; d_tdesc: [max_terms][maxB] the terms' descriptors
    // (PostDesc::voff = the term's value rows).  Compatibility per term (pnp_crf_set_term_compat; holds until changed): d_TM
    // [max_terms] transposed matrices of stride ldm, d_Tvec [max_terms][ldm] vectors
    int max_terms = 0, max_dims = 0;
    bool terms_batch = false;
    int T = 0, tdims[PNP_CRF_MAX_TERMS] = {0};
    PostDesc* d_tdesc = nullptr;
    std::vector<PostDesc> tdesc;
    int tkind[PNP_CRF_MAX_TERMS] = {0}, tcompat_K[PNP_CRF_MAX_TERMS] = {0};
    float *d_TM = nullptr, *d_Tvec = nullptr;
    // -- gradients (pnp_crf_reserve_grad): the workspace of crf_meanfield_backward; q_floats: the row floats of the batch set
    bool grad_reserved = false;
    CrfGradWorkspace gw;
    size_t q_floats = 0;
    std::vector<int> h_tile0;
    // -- pnp_crf_probe_filter on the bilateral term of a two-term batch: the batch's descriptors with voff[0] = voff[1], as
    // crf_slice_add reads a term's value rows (allocated by the first such call)
    PostDesc* d_pdesc = nullptr;
    std::vector<PostDesc> pdesc;
    char err[512] = {0};
};

namespace {

int cfail(pnp_crf* c, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
    return code;
}

#define CHIP(c, call)                                                                          \
    do {                                                                                       \
        hipError_t _s = (call);                                                                \
        if (_s != hipSuccess) return cfail(c, PNP_ERR_HIP, "%s: %s", #call, hipGetErrorString(_s)); \
    } while (0)
#define CK(c, call)                                                                            \
    do {                                                                                       \
        int _r = (call);                                                                       \
        if (_r != PNP_OK) return cfail(c, _r, "%s failed (%d): %s", #call, _r, hipGetErrorString(hipGetLastError())); \
    } while (0)

template <typename T>
int calloc_dev(pnp_crf* c, T** out, size_t count, bool zero = false) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>((count * sizeof(T) + 255) / 256 * 256, 256);
    if (hipMalloc(&p, bytes) != hipSuccess)
        return cfail(c, PNP_ERR_NOMEM, "out of device memory: an allocation of %zu bytes failed with %zu bytes already held", bytes, c->alloc_bytes);
    c->allocs.push_back(p);
    c->alloc_bytes += bytes;
    if (zero && hipMemset(p, 0, bytes) != hipSuccess) return cfail(c, PNP_ERR_HIP, "hipMemset failed");
    *out = reinterpret_cast<T*>(p);
    return PNP_OK;
}

int crf_reserve(pnp_crf* c) {
    const size_t TP = (size_t)c->max_total_pix, B = (size_t)c->maxB;
#define CALLOC(call)                 /* (calloc_dev's message says how many bytes were wanted: kept) */ \
    do {                                                                                               \
        if (int _r = (call)) return _r;                                                                \
    } while (0)
    CALLOC(calloc_dev(c, &c->d_desc, B));
    CALLOC(calloc_dev(c, &c->d_label_off, B + 1));
    CALLOC(calloc_dev(c, &c->d_lut, 256));
    {
        int32_t ident[256];
        for (int i = 0; i < 256; i++) ident[i] = i;
        CHIP(c, hipMemcpy(c->d_lut, ident, sizeof(ident), hipMemcpyHostToDevice));
    }
    for (const CrfAlloc& a : crf_reserve_plan(c->ws, B, TP, TP, (size_t)c->maxKp, 1, (size_t)c->max_terms, (size_t)c->max_dims))
        CALLOC(calloc_dev(c, reinterpret_cast<char**>(a.dst), a.bytes, a.zero));
    // compatibility matrices, and the KL divergence's per-pixel terms, per-run partials and per-image results
    c->ldm = (c->maxKp + 7) / 8 * 8;
    CALLOC(calloc_dev(c, &c->d_M, 2 * (size_t)c->ldm * c->ldm, true));
    CALLOC(calloc_dev(c, &c->kl_pix, TP));
    CALLOC(calloc_dev(c, &c->kl_part, TP / CRF_KL_RUN + B + 1));
    CALLOC(calloc_dev(c, &c->kl_out, B));
    if (c->max_terms) {
        CALLOC(calloc_dev(c, &c->d_tdesc, (size_t)c->max_terms * B));
        CALLOC(calloc_dev(c, &c->d_TM, (size_t)c->max_terms * c->ldm * c->ldm, true));
        CALLOC(calloc_dev(c, &c->d_Tvec, (size_t)c->max_terms * c->ldm, true));
    }
#undef CALLOC
    return PNP_OK;
}

// Host only: validates the batch against the reserved bounds and lays it out (PostDesc, one channel group per row)
int crf_layout(pnp_crf* c, const pnp_crf_batch* b) {
    const int B = b->B;
    c->desc.assign(B, PostDesc{});
    c->h_label_off.assign(B + 1, 0);
    c->kp_max = c->maxHW = 0;
    CrfOffsets at;
    for (int i = 0; i < B; i++) {
        PostDesc d{};
        d.H = b->H[i]; d.W = b->W[i]; d.K = b->K[i];
        if (d.H <= 0 || d.W <= 0) return cfail(c, PNP_ERR_ARG, "image %d: bad size %d x %d", i, d.H, d.W);
        if (d.K < 2 || d.K > c->maxK) return cfail(c, PNP_ERR_ARG, "image %d: %d labels, the solver holds 2..%d", i, d.K, c->maxK);
        const int64_t n = (int64_t)d.H * d.W;
        if (n > c->max_pix_img) return cfail(c, PNP_ERR_ARG, "image %d: %d x %d = %lld pixels, reserved %d per image", i, d.H, d.W, (long long)n, c->max_pix_img);
        d.C = d.K; d.has_bg = 0; d.Kg = d.K;
        if (!crf_layout_image(d, 1, at))
            return cfail(c, PNP_ERR_ARG, "image %d: %lld pixels x %d labels exceed the per-image addressing of the mean-field kernels", i, (long long)n, d.K);
        c->desc[i] = d;
        c->h_label_off[i] = (size_t)d.pix0;
        c->kp_max = std::max(c->kp_max, d.Kp);
        c->maxHW = std::max(c->maxHW, (int)n);
    }
    c->h_label_off[B] = (size_t)at.pix;
    c->q_floats = at.qoff;
    if (at.pix > c->max_total_pix) return cfail(c, PNP_ERR_ARG, "batch has %lld pixels, reserved %lld", (long long)at.pix, (long long)c->max_total_pix);
    if (at.voff[1] > c->ws.val_cap || at.voff[0] > c->ws.valg_cap)
        return cfail(c, PNP_ERR_ARG, "batch needs %zu lattice value floats, reserved %zu", at.voff[1], c->ws.val_cap);
    c->B = B;
    return PNP_OK;
}

}  // namespace

namespace {

int crf_create(int32_t device, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image, int32_t max_labels,
               int32_t max_terms, int32_t max_dims, pnp_crf** out) {
    if (!out) return PNP_ERR_ARG;
    *out = nullptr;
    if (device < 0 || max_batch < 1 || max_batch > CRF_MAX_IMAGES || max_total_pixels < 1 || max_pixels_per_image < 1 ||
        max_pixels_per_image > max_total_pixels || max_labels < 2 || max_labels > CRF_MAX_LABELS)
        return PNP_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return PNP_ERR_HIP;
    pnp_crf* c = new pnp_crf();
    c->max_terms = max_terms;
    c->max_dims = max_dims;
    c->device = device;
    c->maxB = max_batch;
    c->max_total_pix = max_total_pixels;
    c->max_pix_img = max_pixels_per_image;
    c->maxK = max_labels;
    c->maxKp = (max_labels + 3) / 4 * 4;
    *out = c;                                     // handed out on failure too: pnp_crf_last_error says why, pnp_crf_destroy frees
    return crf_reserve(c);
}

}  // namespace

extern "C" int pnp_crf_create(int32_t device, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image,
                              int32_t max_labels, pnp_crf** out) {
    return crf_create(device, max_batch, max_total_pixels, max_pixels_per_image, max_labels, 0, 0, out);
}

extern "C" int pnp_crf_create_terms(int32_t device, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image,
                                    int32_t max_labels, int32_t max_terms, int32_t max_dims, pnp_crf** out) {
    if (out) *out = nullptr;
    if (max_terms < 1 || max_terms > PNP_CRF_MAX_TERMS || max_dims < 1 || max_dims > PNP_CRF_MAX_DIMS) return PNP_ERR_ARG;
    return crf_create(device, max_batch, max_total_pixels, max_pixels_per_image, max_labels, max_terms, max_dims, out);
}

extern "C" void pnp_crf_destroy(pnp_crf* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void* p : c->allocs) (void)hipFree(p);
    delete c;
}

extern "C" size_t pnp_crf_allocated_bytes(const pnp_crf* c) { return c ? c->alloc_bytes : 0; }

extern "C" const char* pnp_crf_last_error(const pnp_crf* c) { return c ? c->err : "null solver"; }

namespace {

// The width whose feature reaches furthest in lattice units over this batch (largest extent / width): the one a key-range
// refusal names.  w: n widths; extent: the largest value of each feature.  Equal widths: the first such
int widest_feature(const float* w, const float* extent, int n) {
    int at = 0;
    for (int i = 1; i < n; i++)
        if (extent[i] / w[i] > extent[at] / w[at]) at = i;
    return at;
}

// The value rows of term t (dims[t] + 1 per pixel at most) image by image, into tdesc[t * B + i]; false: beyond the per-image
// addressing of the iteration kernels (24-bit row ids, 32-bit byte offsets: crf_meanfield.hip)
bool crf_layout_terms(pnp_crf* c, int T, const int* dims, size_t* need) {
    const int B = c->B;
    c->tdesc.assign((size_t)T * B, PostDesc{});
    *need = 0;
    for (int t = 0; t < T; t++) {
        size_t voff = 0;
        for (int i = 0; i < B; i++) {
            PostDesc d = c->desc[i];
            const int64_t rows = (int64_t)d.H * d.W * (dims[t] + 1);
            d.voff[0] = d.voff[1] = voff;
            voff += (size_t)rows * d.Kp;
            c->tdesc[(size_t)t * B + i] = d;
            if (rows >= (1 << 24) || rows * d.Kp * 4 >= ((int64_t)1 << 32)) return false;
        }
        *need = std::max(*need, voff);
    }
    return true;
}

// Both forms of set_batch, once the caller's own arguments are through (b non-null; the state flags went down as the call
// began): B range, null arrays (`arrays`: the caller's are there), the caller's later checks (`own`), the layout -- of T feature
// terms too --, then on the stream the descriptors, the label offsets and the unary planes into rows
template <typename Own>
int crf_batch_prologue(pnp_crf* c, const pnp_crf_batch* b, bool arrays, const char* arrays_msg, Own own, int T, const int* dims, hipStream_t s) {
    if (b->B < 1 || b->B > c->maxB) return cfail(c, PNP_ERR_ARG, "batch of %d images, the solver holds 1..%d", b->B, c->maxB);
    if (!arrays) return cfail(c, PNP_ERR_ARG, "%s", arrays_msg);
    if (int r = own()) return r;
    if (int r = crf_layout(c, b)) return r;
    if (T) {
        size_t need = 0;
        if (!crf_layout_terms(c, T, dims, &need))
            return cfail(c, PNP_ERR_ARG, "an image's lattice value rows exceed the per-image addressing of the mean-field kernels");
        if (need > c->ws.val_cap) return cfail(c, PNP_ERR_ARG, "batch needs %zu lattice value floats, reserved %zu", need, c->ws.val_cap);
    }
    CHIP(c, hipSetDevice(c->device));
    const int B = c->B;
    // (pageable host memory: copied into the runtime's staging buffer at enqueue time, so the vectors may be rewritten by the
    // next call without a synchronisation)
    CHIP(c, hipMemcpyAsync(c->d_desc, c->desc.data(), sizeof(PostDesc) * B, hipMemcpyHostToDevice, s));
    for (int t = 0; t < T; t++)
        CHIP(c, hipMemcpyAsync(c->d_tdesc + (size_t)t * c->maxB, c->tdesc.data() + (size_t)t * B, sizeof(PostDesc) * B, hipMemcpyHostToDevice, s));
    CHIP(c, hipMemcpyAsync(c->d_label_off, c->h_label_off.data(), sizeof(size_t) * (B + 1), hipMemcpyHostToDevice, s));
    CK(c, crf_planes_rows(true, c->d_desc, const_cast<float*>(b->d_unary), c->ws.unary, B, c->maxHW, c->kp_max, s));
    return PNP_OK;
}

// pnp_crf_set_batch / pnp_crf_set_batch_aniso: pos_xy = (sx, sy) of the Gaussian term, bi_xy / bi_rgb = (sx, sy) / (sr, sg, sb)
// of the bilateral one
int crf_set_batch(pnp_crf* c, const pnp_crf_batch* b, const float pos_xy[2], const float bi_xy[2], const float bi_rgb[3], void* stream) {
    c->ready = c->started = false;
    if (!c->ws.va || !c->kl_out) return cfail(c, PNP_ERR_STATE, "the solver's workspace was not allocated (pnp_crf_create failed)");
    if (!b) return cfail(c, PNP_ERR_ARG, "batch is null");
    const bool iso = pos_xy[0] == pos_xy[1] && bi_xy[0] == bi_xy[1] && bi_rgb[0] == bi_rgb[1] && bi_rgb[0] == bi_rgb[2];
    auto widths = [&] {
        if ((pos_xy[0] > 0.f) && (pos_xy[1] > 0.f) && (bi_xy[0] > 0.f) && (bi_xy[1] > 0.f) && (bi_rgb[0] > 0.f) && (bi_rgb[1] > 0.f) &&
            (bi_rgb[2] > 0.f))
            return (int)PNP_OK;
        if (iso) return cfail(c, PNP_ERR_ARG, "kernel widths must be positive (pos_xy=%g, bi_xy=%g, bi_rgb=%g)", pos_xy[0], bi_xy[0], bi_rgb[0]);
        return cfail(c, PNP_ERR_ARG, "kernel widths must be positive (pos_xy=(%g, %g), bi_xy=(%g, %g), bi_rgb=(%g, %g, %g))", pos_xy[0],
                     pos_xy[1], bi_xy[0], bi_xy[1], bi_rgb[0], bi_rgb[1], bi_rgb[2]);
    };
    hipStream_t s = (hipStream_t)stream;
    if (int r = crf_batch_prologue(c, b, b->H && b->W && b->K && b->d_rgb && b->d_unary, "batch has null arrays (H, W, K, d_rgb, d_unary)",
                                   widths, 0, nullptr, s))
        return r;
    const int B = c->B;
    int range_term = -1;
    const int built = crf_build(c->ws, c->d_desc, c->desc.data(), B, c->h_label_off[B], c->maxHW, b->d_rgb, pos_xy, bi_xy, bi_rgb, &range_term, s);
    if (range_term >= 0) {
        // the flag says that a coordinate left the key, not which feature drove it there: named is the width whose feature
        // spans the most lattice units over these images
        float extent[5] = {0.f, 0.f, 255.f, 255.f, 255.f};
        for (const PostDesc& d : c->desc) {
            extent[0] = std::max(extent[0], (float)(d.W - 1));
            extent[1] = std::max(extent[1], (float)(d.H - 1));
        }
        if (range_term == 0) {
            if (iso)
                return cfail(c, built, "lattice key range exceeded: a Gaussian coordinate leaves the 16-bit key; pos_xy = %g is too small for these images", pos_xy[0]);
            const int at = widest_feature(pos_xy, extent, 2);
            return cfail(c, built, "lattice key range exceeded: a Gaussian coordinate leaves the 16-bit key; pos_xy[%d] = %g is too small for these images", at, pos_xy[at]);
        }
        if (iso)
            return cfail(c, built,
                         "lattice key range exceeded: a bilateral coordinate leaves the 11-bit key (|coordinate| must stay below %d); "
                         "bi_rgb = %g (bi_xy = %g) is too small for these images",
                         CRF_KEY_LIMIT, bi_rgb[0], bi_xy[0]);
        const float w5[5] = {bi_xy[0], bi_xy[1], bi_rgb[0], bi_rgb[1], bi_rgb[2]};
        const int at = widest_feature(w5, extent, 5);
        return cfail(c, built,
                     "lattice key range exceeded: a bilateral coordinate leaves the 11-bit key (|coordinate| must stay below %d); "
                     "%s[%d] = %g is too small for these images (bi_xy = (%g, %g), bi_rgb = (%g, %g, %g))",
                     CRF_KEY_LIMIT, at < 2 ? "bi_xy" : "bi_rgb", at < 2 ? at : at - 2, w5[at], w5[0], w5[1], w5[2], w5[3], w5[4]);
    }
    if (built != PNP_OK) return cfail(c, built, "lattice build failed (%d): %s", built, hipGetErrorString(hipGetLastError()));
    c->ready = true;
    c->terms_batch = false;
    return PNP_OK;
}

}  // namespace

extern "C" int pnp_crf_set_batch_terms(pnp_crf* c, const pnp_crf_batch* b, int32_t n_terms, const pnp_crf_term* terms, void* stream) {
    if (!c) return PNP_ERR_ARG;
    c->ready = false;
    c->started = false;
    if (!b) return cfail(c, PNP_ERR_ARG, "batch is null");
    if (!terms) return cfail(c, PNP_ERR_ARG, "the term array is null");
    if (n_terms < 1 || n_terms > PNP_CRF_MAX_TERMS) return cfail(c, PNP_ERR_ARG, "%d terms: 1..%d", n_terms, PNP_CRF_MAX_TERMS);
    int dims[PNP_CRF_MAX_TERMS];
    const float* feat[PNP_CRF_MAX_TERMS];
    for (int t = 0; t < n_terms; t++) {
        if (terms[t].dims < 1 || terms[t].dims > PNP_CRF_MAX_DIMS)
            return cfail(c, PNP_ERR_ARG, "term %d has %d feature axes: 1..%d", t, terms[t].dims, PNP_CRF_MAX_DIMS);
        if (!terms[t].d_features) return cfail(c, PNP_ERR_ARG, "term %d: d_features is null", t);
        dims[t] = terms[t].dims;
        feat[t] = terms[t].d_features;
    }
    if (!c->max_terms) return cfail(c, PNP_ERR_STATE, "this solver holds no feature terms: create it with pnp_crf_create_terms");
    if (!c->ws.va || !c->d_Tvec) return cfail(c, PNP_ERR_STATE, "the solver's workspace was not allocated (pnp_crf_create_terms failed)");
    if (n_terms > c->max_terms) return cfail(c, PNP_ERR_ARG, "%d terms, the solver holds 1..%d", n_terms, c->max_terms);
    for (int t = 0; t < n_terms; t++)
        if (dims[t] > c->max_dims) return cfail(c, PNP_ERR_ARG, "term %d has %d feature axes, the solver holds 1..%d", t, dims[t], c->max_dims);
    hipStream_t s = (hipStream_t)stream;
    if (int r = crf_batch_prologue(c, b, b->H && b->W && b->K && b->d_unary, "batch has null arrays (H, W, K, d_unary)", [] { return (int)PNP_OK; },
                                   n_terms, dims, s))
        return r;
    const int B = c->B;
    int range_term = -1;
    const int built = crf_build_terms(c->ws, c->d_desc, c->desc.data(), B, c->h_label_off[B], c->maxHW, n_terms, dims, feat, &range_term, s);
    if (range_term >= 0)
        return cfail(c, built,
                     "lattice key range exceeded: term %d (%d feature axes) has a lattice coordinate beyond the key (|coordinate| must stay "
                     "below %d for %d axes) or a feature that is not finite; a wider kernel width (smaller features) is the remedy",
                     range_term, dims[range_term], crf_feature_key_limit(dims[range_term]), dims[range_term]);
    if (built != PNP_OK) return cfail(c, built, "lattice build failed (%d): %s", built, hipGetErrorString(hipGetLastError()));
    c->T = n_terms;
    for (int t = 0; t < n_terms; t++) c->tdims[t] = dims[t];
    c->ready = true;
    c->terms_batch = true;
    return PNP_OK;
}

extern "C" int64_t pnp_crf_lattice_points(const pnp_crf* c, int32_t term) {
    if (!c || !c->ready || term < 0 || term >= (c->terms_batch ? c->T : 2)) return -1;
    return c->terms_batch ? c->ws.tlat_points[term] : c->ws.lat_points[term];
}

namespace {

// A vector or matrix compatibility of K labels from the host to the device: the checks, then a matrix TRANSPOSED into d_matrix
// (stride ldm), a diagonal as a vector of ldm floats into d_vector or -- d_vector null: the two-term solver's -- as a matrix.
// d_matrix null: the workspace that `creator` allocates is not there
int crf_upload_compat(pnp_crf* c, int kind, const float* host_values, int K, const char* creator, float* d_matrix, float* d_vector) {
    if (kind != PNP_CRF_COMPAT_DIAGONAL && kind != PNP_CRF_COMPAT_MATRIX)
        return cfail(c, PNP_ERR_ARG, "kind = %d: scalar (0), diagonal (1) or matrix (2)", kind);
    if (!host_values) return cfail(c, PNP_ERR_ARG, "compatibility values are null");
    if (K < 2 || K > c->maxK) return cfail(c, PNP_ERR_ARG, "compatibility for %d labels, the solver holds 2..%d", K, c->maxK);
    if (!d_matrix) return cfail(c, PNP_ERR_STATE, "the solver's workspace was not allocated (%s failed)", creator);
    const size_t ld = (size_t)c->ldm;
    const bool diag = kind == PNP_CRF_COMPAT_DIAGONAL, vec = diag && d_vector;
    c->h_M.assign(vec ? ld : ld * ld, 0.f);
    for (int l = 0; l < K; l++) {
        if (diag) c->h_M[vec ? l : l * ld + l] = host_values[l];
        else
            for (int k = 0; k < K; k++) c->h_M[k * ld + l] = host_values[(size_t)l * K + k];      // (transposed)
    }
    CHIP(c, hipSetDevice(c->device));
    // (synchronous: the weights may not change under a step still in flight, and host_values may be freed on return)
    CHIP(c, hipDeviceSynchronize());
    CHIP(c, hipMemcpy(vec ? d_vector : d_matrix, c->h_M.data(), sizeof(float) * c->h_M.size(), hipMemcpyHostToDevice));
    return PNP_OK;
}

}  // namespace

extern "C" int pnp_crf_set_term_compat(pnp_crf* c, int32_t term, int32_t kind, const float* host_values, int32_t K) {
    if (!c) return PNP_ERR_ARG;
    if (term < 0 || term >= PNP_CRF_MAX_TERMS || term >= c->max_terms)
        return cfail(c, PNP_ERR_ARG, "term = %d: the solver holds terms 0..%d (pnp_crf_create_terms)", term, c->max_terms - 1);
    if (kind == PNP_CRF_COMPAT_SCALAR) {          // the weight of the call; the values are not read
        c->tkind[term] = kind;
        c->tcompat_K[term] = 0;
        return PNP_OK;
    }
    const size_t ld = (size_t)c->ldm;
    const bool have = c->d_TM && c->d_Tvec;
    if (int r = crf_upload_compat(c, kind, host_values, K, "pnp_crf_create_terms", have ? c->d_TM + term * ld * ld : nullptr,
                                  have ? c->d_Tvec + term * ld : nullptr))
        return r;
    c->tkind[term] = kind;
    c->tcompat_K[term] = K;
    return PNP_OK;
}

extern "C" int pnp_crf_set_batch(pnp_crf* c, const pnp_crf_batch* b, float pos_xy, float bi_xy, float bi_rgb, void* stream) {
    if (!c) return PNP_ERR_ARG;
    const float p2[2] = {pos_xy, pos_xy}, b2[2] = {bi_xy, bi_xy}, b3[3] = {bi_rgb, bi_rgb, bi_rgb};
    return crf_set_batch(c, b, p2, b2, b3, stream);
}

extern "C" int pnp_crf_set_batch_aniso(pnp_crf* c, const pnp_crf_batch* b, const float pos_xy[2], const float bi_xy[2],
                                       const float bi_rgb[3], void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (!pos_xy || !bi_xy || !bi_rgb) {
        c->ready = c->started = false;
        return cfail(c, PNP_ERR_ARG, "kernel widths are null (pos_xy[2], bi_xy[2], bi_rgb[3])");
    }
    return crf_set_batch(c, b, pos_xy, bi_xy, bi_rgb, stream);
}

extern "C" int pnp_crf_set_compat(pnp_crf* c, int32_t term, int32_t kind, const float* host_values, int32_t K) {
    if (!c) return PNP_ERR_ARG;
    if (term != 0 && term != 1) return cfail(c, PNP_ERR_ARG, "term = %d: 0 (Gaussian) or 1 (bilateral)", term);
    if (kind == PNP_CRF_COMPAT_SCALAR) {          // back to Potts with the weight of the call; the values are not read
        c->kind[term] = kind;
        c->compat_K[term] = 0;
        c->m_scalar[term] = false;
        return PNP_OK;
    }
    const size_t ld = (size_t)c->ldm;
    if (int r = crf_upload_compat(c, kind, host_values, K, "pnp_crf_create", c->d_M ? c->d_M + term * ld * ld : nullptr, nullptr)) return r;
    c->kind[term] = kind;
    c->compat_K[term] = K;
    c->m_scalar[term] = false;
    return PNP_OK;
}

namespace {

int crf_need_batch(pnp_crf* c) {
    if (!c->ready) return cfail(c, PNP_ERR_STATE, "no batch is set: call pnp_crf_set_batch first (a failed call leaves none)");
    return PNP_OK;
}

// The two kinds of batch have their own inference calls (pnp_crf_start and pnp_crf_read serve both)
int crf_need_kind(pnp_crf* c, bool terms, const char* call) {
    if (c->terms_batch == terms) return PNP_OK;
    if (terms) return cfail(c, PNP_ERR_STATE, "%s needs a batch of pnp_crf_set_batch_terms; the batch set is a two-term one (pnp_crf_infer / _step)", call);
    return cfail(c, PNP_ERR_STATE, "%s needs a two-term batch (pnp_crf_set_batch); the batch set has feature terms (pnp_crf_infer_terms / _step_terms)", call);
}

// A vector or matrix compatibility fixes the label count of the batch: every image has the K it was set for.  whose: the
// term as the message names it
int crf_compat_labels(pnp_crf* c, const char* whose, int K) {
    for (int i = 0; i < c->B; i++)
        if (c->desc[i].K != K)
            return cfail(c, PNP_ERR_ARG, "%s's compatibility is for %d labels, image %d of the batch has %d: a vector or matrix "
                         "compatibility needs that many labels in every image", whose, K, i, c->desc[i].K);
    return PNP_OK;
}

// Both terms as matrices on the device: a term left scalar as w * I
int crf_matrices(pnp_crf* c, float pos_w, float bi_w, hipStream_t s) {
    const size_t ld = (size_t)c->ldm;
    for (int t = 0; t < 2; t++) {
        if (c->kind[t] != PNP_CRF_COMPAT_SCALAR) {
            if (int r = crf_compat_labels(c, t == 0 ? "the Gaussian term" : "the bilateral term", c->compat_K[t])) return r;
            continue;
        }
        const float w = t == 0 ? pos_w : bi_w;
        if (c->m_scalar[t] && c->m_scalar_w[t] == w) continue;
        c->h_M.assign(ld * ld, 0.f);
        for (size_t l = 0; l < ld; l++) c->h_M[l * ld + l] = w;
        // (pageable host memory is staged at enqueue time: h_M may be rewritten by the next term)
        CHIP(c, hipMemcpyAsync(c->d_M + t * ld * ld, c->h_M.data(), sizeof(float) * ld * ld, hipMemcpyHostToDevice, s));
        c->m_scalar[t] = true;
        c->m_scalar_w[t] = w;
    }
    return PNP_OK;
}

CrfLabelOut crf_labels(pnp_crf* c, uint8_t* d_labels) {
    // labels: the argmax the last update does on the marginals it has just normalised (first maximum, a NaN wins), through
    // the identity table (stride 0: the same table for every image)
    CrfLabelOut lab;
    if (d_labels) {
        lab.lab[0] = d_labels;
        lab.lut = c->d_lut;
        lab.lut_stride = 0;
        lab.label_off = c->d_label_off;
    }
    return lab;
}

CrfSpan crf_span(const pnp_crf* c) { return CrfSpan{c->d_desc, 0, c->B, c->kp_max, 1}; }

// Q0 = softmax(-U)
int crf_start(pnp_crf* c, hipStream_t s, const CrfLabelOut& lab) {
    CK(c, crf_meanfield_start(c->ws, crf_span(c), s, lab));
    c->started = true;
    return PNP_OK;
}

// n mean-field updates from the current Q: the Potts kernel while both terms are scalar, the compatibility kernel otherwise.
// lab: label output of the last update
int crf_step(pnp_crf* c, int n, float pos_w, float bi_w, hipStream_t s, const CrfLabelOut& lab) {
    const bool potts = c->kind[0] == PNP_CRF_COMPAT_SCALAR && c->kind[1] == PNP_CRF_COMPAT_SCALAR;
    const size_t ld = (size_t)c->ldm;
    if (!potts && n > 0)
        if (int r = crf_matrices(c, pos_w, bi_w, s)) return r;
    CK(c, crf_meanfield(c->ws, crf_span(c), n, CrfPairRun{pos_w, bi_w, potts ? nullptr : c->d_M, c->d_M + ld * ld, (int)ld}, s, lab));
    return PNP_OK;
}

// The marginals out: the rows of Q into the caller's planes (d_q null: not asked for)
int crf_emit_q(pnp_crf* c, float* d_q, hipStream_t s) {
    if (d_q) CK(c, crf_planes_rows(false, c->d_desc, d_q, c->ws.Q, c->B, c->maxHW, c->kp_max, s));
    return PNP_OK;
}

// What crf_meanfield_terms / crf_meanfield_backward take of the T terms of the batch (`run`), and the arrays it points into:
// descriptors and compatibilities per term.  weights[t]: the weight of a term left scalar
struct CrfTermsArgs {
    const PostDesc* desc[PNP_CRF_MAX_TERMS];
    const float *wvec[PNP_CRF_MAX_TERMS], *MT[PNP_CRF_MAX_TERMS];
    CrfTermsRun run;
    int fill(pnp_crf* c, const float* weights) {
        const size_t ld = (size_t)c->ldm;
        for (int t = 0; t < c->T; t++) {
            char whose[16];
            snprintf(whose, sizeof(whose), "term %d", t);
            if (c->tkind[t] != PNP_CRF_COMPAT_SCALAR)
                if (int r = crf_compat_labels(c, whose, c->tcompat_K[t])) return r;
            desc[t] = c->d_tdesc + (size_t)t * c->maxB;
            wvec[t] = c->tkind[t] == PNP_CRF_COMPAT_DIAGONAL ? c->d_Tvec + t * ld : nullptr;
            MT[t] = c->tkind[t] == PNP_CRF_COMPAT_MATRIX ? c->d_TM + t * ld * ld : nullptr;
        }
        run = CrfTermsRun{c->T, desc, weights, wvec, MT, c->ldm};
        return PNP_OK;
    }
};

// n updates of the T feature terms from the current Q
int crf_step_terms(pnp_crf* c, int n, const float* weights, hipStream_t s, const CrfLabelOut& lab) {
    CrfTermsArgs a;
    if (int r = a.fill(c, weights)) return r;
    CK(c, crf_meanfield_terms(c->ws, crf_span(c), n, a.run, s, lab));
    return PNP_OK;
}

// pnp_crf_infer_terms (`call`), and pnp_crf_infer_terms_saved (saved): the same launches one update at a time, the rows of Q
// copied out to d_history in between
int crf_infer_terms(pnp_crf* c, const char* call, bool saved, int32_t iters, const float* weights, float* d_history, float* d_q,
                    uint8_t* d_labels, void* stream) {
    if (iters < 0) return cfail(c, PNP_ERR_ARG, "iters = %d", iters);
    if (!weights) return cfail(c, PNP_ERR_ARG, "weights is null (one float per term)");
    if (saved && !d_history) return cfail(c, PNP_ERR_ARG, "d_history is null (iters + 1 blocks of the batch's row floats)");
    if (int r = crf_need_batch(c)) return r;
    if (int r = crf_need_kind(c, true, call)) return r;
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    const CrfLabelOut lab = crf_labels(c, d_labels);
    const size_t qbytes = c->q_floats * sizeof(float);
    if (int r = crf_start(c, s, iters == 0 ? lab : CrfLabelOut())) return r;
    if (!saved) {
        if (int r = crf_step_terms(c, iters, weights, s, lab)) return r;
        return crf_emit_q(c, d_q, s);
    }
    CHIP(c, hipMemcpyAsync(d_history, c->ws.Q, qbytes, hipMemcpyDeviceToDevice, s));
    for (int it = 1; it <= iters; it++) {
        if (int r = crf_step_terms(c, 1, weights, s, it == iters ? lab : CrfLabelOut())) return r;
        CHIP(c, hipMemcpyAsync(d_history + (size_t)it * c->q_floats, c->ws.Q, qbytes, hipMemcpyDeviceToDevice, s));
    }
    return crf_emit_q(c, d_q, s);
}

}  // namespace

extern "C" int pnp_crf_infer_terms(pnp_crf* c, int32_t iters, const float* weights, float* d_q, uint8_t* d_labels, void* stream) {
    if (!c) return PNP_ERR_ARG;
    return crf_infer_terms(c, "pnp_crf_infer_terms", false, iters, weights, nullptr, d_q, d_labels, stream);
}

extern "C" int pnp_crf_infer_terms_saved(pnp_crf* c, int32_t iters, const float* weights, float* d_history, float* d_q, uint8_t* d_labels,
                                         void* stream) {
    if (!c) return PNP_ERR_ARG;
    return crf_infer_terms(c, "pnp_crf_infer_terms_saved", true, iters, weights, d_history, d_q, d_labels, stream);
}

extern "C" int pnp_crf_reserve_grad(pnp_crf* c) {
    if (!c) return PNP_ERR_ARG;
    if (!c->max_terms) return cfail(c, PNP_ERR_STATE, "gradients serve solvers of feature terms: create it with pnp_crf_create_terms");
    if (!c->ws.va || !c->d_Tvec) return cfail(c, PNP_ERR_STATE, "the solver's workspace was not allocated (pnp_crf_create_terms failed)");
    if (c->grad_reserved) return PNP_OK;
    CHIP(c, hipSetDevice(c->device));
    const size_t TP = (size_t)c->max_total_pix, B = (size_t)c->maxB, rows = TP * c->maxKp;
    CrfGradWorkspace& gw = c->gw;
    // partials: a quarter more tiles than the batch's pixels fill at the widest rows' tile (ragged image edges), a few per image;
    // a batch with more tiles (thin images, 1-D signals) goes through the buffer in spans (crf_meanfield_backward)
    size_t smem = 0;
    const size_t tp = (size_t)crf_backward_tile_pixels(c->maxKp, &smem);
    gw.max_psz = (size_t)c->maxK * c->maxK;
    gw.part_cap = (TP / tp + TP / (4 * tp) + 2 * B + 16) * gw.max_psz;
    // Nothing is zero-filled: every array is written in full before it is read -- the rows of g and gU, pad floats included, by
    // crf_planes_rows / hipMemsetAsync, those of dl and h by the kernels that own them, the partials and sums tile by tile.
    // An array is allocated only while its pointer is null, so a call after one that ran out of memory allocates the rest
    auto want = [c](auto** p, size_t count) { return *p ? PNP_OK : calloc_dev(c, p, count); };
    for (float** p : {&gw.g, &gw.dl, &gw.h, &gw.gU})
        if (int r = want(p, rows)) return r;
    if (int r = want(&gw.part, gw.part_cap)) return r;
    if (int r = want(&gw.img_sum, B * gw.max_psz)) return r;
    if (int r = want(&gw.acc, (size_t)c->max_terms * gw.max_psz)) return r;
    if (int r = want(&gw.tile0, B + 1)) return r;
    c->grad_reserved = true;
    return PNP_OK;
}

extern "C" int pnp_crf_backward_terms(pnp_crf* c, int32_t iters, const float* weights, const float* d_history, const float* d_grad_q,
                                      float* d_grad_unary, float* const* d_grad_compat, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (iters < 0) return cfail(c, PNP_ERR_ARG, "iters = %d", iters);
    if (!weights) return cfail(c, PNP_ERR_ARG, "weights is null (one float per term)");
    if (!d_history || !d_grad_q || !d_grad_unary) return cfail(c, PNP_ERR_ARG, "null pointers (d_history, d_grad_q, d_grad_unary)");
    if (int r = crf_need_batch(c)) return r;
    if (int r = crf_need_kind(c, true, "pnp_crf_backward_terms")) return r;
    if (!c->grad_reserved) return cfail(c, PNP_ERR_STATE, "the gradient workspace is not allocated: call pnp_crf_reserve_grad first");
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    CrfTermsArgs a;
    if (int r = a.fill(c, weights)) return r;
    int psz[PNP_CRF_MAX_TERMS] = {0};
    for (int t = 0; t < c->T; t++) {
        if (!d_grad_compat || !d_grad_compat[t]) continue;
        const int K = c->tcompat_K[t];
        psz[t] = c->tkind[t] == PNP_CRF_COMPAT_MATRIX ? K * K : c->tkind[t] == PNP_CRF_COMPAT_DIAGONAL ? K : 1;
    }
    size_t smem = 0;
    const int tp = crf_backward_tile_pixels(c->kp_max, &smem);
    c->h_tile0.assign(c->B + 1, 0);
    for (int i = 0; i < c->B; i++) c->h_tile0[i + 1] = c->h_tile0[i] + crf_backward_tiles(c->desc[i].H, c->desc[i].W, tp);
    // (pageable host memory is staged at enqueue time: h_tile0 may be rewritten by the next call)
    CHIP(c, hipMemcpyAsync(c->gw.tile0, c->h_tile0.data(), sizeof(int) * (c->B + 1), hipMemcpyHostToDevice, s));
    CK(c, crf_planes_rows(true, c->d_desc, const_cast<float*>(d_grad_q), c->gw.g, c->B, c->maxHW, c->kp_max, s));
    CK(c, crf_meanfield_backward(c->ws, c->gw, crf_span(c), c->maxHW, iters, a.run, d_history, c->q_floats, psz, c->h_tile0.data(), s));
    CK(c, crf_planes_rows(false, c->d_desc, d_grad_unary, c->gw.gU, c->B, c->maxHW, c->kp_max, s));
    for (int t = 0; t < c->T; t++)
        if (psz[t]) CK(c, crf_grad_emit(c->gw.acc + (size_t)t * c->gw.max_psz, psz[t], d_grad_compat[t], s));
    return PNP_OK;
}

extern "C" int pnp_crf_step_terms(pnp_crf* c, int32_t n, const float* weights, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (n < 0) return cfail(c, PNP_ERR_ARG, "n = %d", n);
    if (!weights) return cfail(c, PNP_ERR_ARG, "weights is null (one float per term)");
    if (int r = crf_need_batch(c)) return r;
    if (int r = crf_need_kind(c, true, "pnp_crf_step_terms")) return r;
    if (!c->started) return cfail(c, PNP_ERR_STATE, "no inference was started on this batch: call pnp_crf_start (or pnp_crf_infer_terms) first");
    CHIP(c, hipSetDevice(c->device));
    return crf_step_terms(c, n, weights, (hipStream_t)stream, CrfLabelOut());
}

extern "C" int pnp_crf_infer(pnp_crf* c, int32_t iters, float pos_w, float bi_w, float* d_q, uint8_t* d_labels, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (iters < 0) return cfail(c, PNP_ERR_ARG, "iters = %d", iters);
    if (int r = crf_need_batch(c)) return r;
    if (int r = crf_need_kind(c, false, "pnp_crf_infer")) return r;
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    // pnp_crf_start + pnp_crf_step(iters) with the labels fused into the last update, then the marginals out
    const CrfLabelOut lab = crf_labels(c, d_labels);
    if (int r = crf_start(c, s, iters == 0 ? lab : CrfLabelOut())) return r;
    if (int r = crf_step(c, iters, pos_w, bi_w, s, lab)) return r;
    return crf_emit_q(c, d_q, s);
}

extern "C" int pnp_crf_start(pnp_crf* c, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (int r = crf_need_batch(c)) return r;
    CHIP(c, hipSetDevice(c->device));
    return crf_start(c, (hipStream_t)stream, CrfLabelOut());
}

extern "C" int pnp_crf_step(pnp_crf* c, int32_t n, float pos_w, float bi_w, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (n < 0) return cfail(c, PNP_ERR_ARG, "n = %d", n);
    if (int r = crf_need_batch(c)) return r;
    if (int r = crf_need_kind(c, false, "pnp_crf_step")) return r;
    if (!c->started) return cfail(c, PNP_ERR_STATE, "no inference was started on this batch: call pnp_crf_start (or pnp_crf_infer) first");
    CHIP(c, hipSetDevice(c->device));
    return crf_step(c, n, pos_w, bi_w, (hipStream_t)stream, CrfLabelOut());
}

extern "C" int pnp_crf_read(pnp_crf* c, float* d_q, uint8_t* d_labels, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (int r = crf_need_batch(c)) return r;
    if (!c->started) return cfail(c, PNP_ERR_STATE, "no inference was started on this batch: call pnp_crf_start (or pnp_crf_infer) first");
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    if (int r = crf_emit_q(c, d_q, s)) return r;
    if (d_labels) CK(c, argmax_remap(c->ws.Q, c->d_desc, c->d_lut, 0, d_labels, c->d_label_off, 1, 0, c->B, c->maxHW, s));
    return PNP_OK;
}

extern "C" int pnp_crf_kl(pnp_crf* c, float pos_w, float bi_w, double* h_out_per_image, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (!h_out_per_image) return cfail(c, PNP_ERR_ARG, "h_out_per_image is null");
    if (int r = crf_need_batch(c)) return r;
    if (c->terms_batch) return cfail(c, PNP_ERR_ARG, "the KL divergence is not available for a batch of feature terms (pnp_crf_set_batch_terms)");
    if (!c->started) return cfail(c, PNP_ERR_STATE, "no inference was started on this batch: call pnp_crf_start (or pnp_crf_infer) first");
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    if (int r = crf_matrices(c, pos_w, bi_w, s)) return r;
    const size_t ld = (size_t)c->ldm;
    const float *rg = nullptr, *rb = nullptr;                // one filter pass per term at the current Q, which stays as it is
    CK(c, crf_meanfield_filter(c->ws, crf_span(c), &rg, &rb, s));
    CK(c, crf_update_compat(c->ws.lat[0], c->ws.lat[1], c->d_desc, 0, c->B, rg, rb, c->ws.norm[0], c->ws.norm[1], c->ws.unary, c->ws.Q, c->d_M,
                            c->d_M + ld * ld, (int)ld, c->kp_max, s, CrfLabelOut(), c->kl_pix));
    const int runs = (c->maxHW + CRF_KL_RUN - 1) / CRF_KL_RUN;
    hipLaunchKernelGGL(crf_kl_partial_kernel, dim3(runs < 1024 ? runs : 1024, c->B), dim3(CRF_KL_RUN), 0, s, c->d_desc, c->kl_pix, c->kl_part);
    hipLaunchKernelGGL(crf_kl_final_kernel, dim3(1), dim3(64), 0, s, c->d_desc, c->kl_part, c->kl_out, c->B);
    CHIP(c, hipGetLastError());
    CHIP(c, hipMemcpyAsync(h_out_per_image, c->kl_out, sizeof(double) * c->B, hipMemcpyDeviceToHost, s));
    CHIP(c, hipStreamSynchronize(s));
    return PNP_OK;
}

// ------------------------------------------------------------------------------------------ a term's lattice, stage by stage
namespace {

// term of the batch that is set -> its lattice and normaliser; errors as pnp_crf_lattice_points' callers expect them
int crf_term_lattice(pnp_crf* c, int32_t term, const CrfLattice** L, const float** norm) {
    if (int r = crf_need_batch(c)) return r;
    const int T = c->terms_batch ? c->T : 2;
    if (term < 0 || term >= T) return cfail(c, PNP_ERR_ARG, "term = %d: the batch has terms 0..%d", term, T - 1);
    *L = c->terms_batch ? &c->ws.tlat[term] : &c->ws.lat[term];
    *norm = c->terms_batch ? c->ws.tnorm[term] : c->ws.norm[term];
    return PNP_OK;
}

}  // namespace

extern "C" int pnp_crf_lattice_view_get(pnp_crf* c, int32_t term, pnp_crf_lattice_view* out) {
    if (!c) return PNP_ERR_ARG;
    if (!out) return cfail(c, PNP_ERR_ARG, "the view is null");
    const CrfLattice* L = nullptr;
    const float* norm = nullptr;
    if (int r = crf_term_lattice(c, term, &L, &norm)) return r;
    out->D1 = L->D1;
    out->images = c->B;
    out->cap = (int64_t)L->cap;
    out->points = c->terms_batch ? c->ws.tlat_points[term] : c->ws.lat_points[term];
    out->entries = (int64_t)c->h_label_off[c->B] * L->D1;
    out->bary = L->bary;
    out->offset = L->offset;
    out->vals = L->vals;
    out->ent = L->ent;
    out->seg_lo = L->seg_lo;
    out->seg_hi = L->seg_hi;
    out->idbase = L->idbase;
    out->n1 = L->n1;
    out->n2 = L->n2;
    out->nbr8 = L->nbr8;
    out->norm = norm;
    return PNP_OK;
}

extern "C" int pnp_crf_probe_filter(pnp_crf* c, int32_t term, int32_t stage, const float* d_in, float* d_out, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (stage < PNP_CRF_PROBE_SPLAT || stage > PNP_CRF_PROBE_SLICE)
        return cfail(c, PNP_ERR_ARG, "stage = %d: splat (0), forward (1), reverse (2) or slice (3)", stage);
    if (!d_in || !d_out) return cfail(c, PNP_ERR_ARG, "null pointers (d_in, d_out)");
    const CrfLattice* L = nullptr;
    const float* norm = nullptr;
    if (int r = crf_term_lattice(c, term, &L, &norm)) return r;
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    const int B = c->B;
    // the term's descriptors: PostDesc::voff[L->which] = its value rows for the filter, voff[0] for crf_slice_add
    const PostDesc* desc = c->d_desc;
    if (c->terms_batch) {
        desc = c->d_tdesc + (size_t)term * c->maxB;
    } else if (term == 1) {
        if (!c->d_pdesc)
            if (int r = calloc_dev(c, &c->d_pdesc, (size_t)c->maxB)) return r;
        c->pdesc = c->desc;
        for (PostDesc& d : c->pdesc) d.voff[0] = d.voff[1];
        // (pageable host memory is staged at enqueue time: pdesc may be rewritten by the next call)
        CHIP(c, hipMemcpyAsync(c->d_pdesc, c->pdesc.data(), sizeof(PostDesc) * B, hipMemcpyHostToDevice, s));
        desc = c->d_pdesc;
    }
    const bool gauss = !c->terms_batch && term == 0;
    float* const va = gauss ? c->ws.vga : c->ws.va;
    float* const vb = gauss ? c->ws.vgb : c->ws.vb;
    c->started = false;                           // Q holds the caller's rows from here on
    CK(c, crf_planes_rows(true, c->d_desc, const_cast<float*>(d_in), c->ws.Q, B, c->maxHW, c->kp_max, s));
    const float* val = nullptr;
    CK(c, crf_filter(*L, desc, 0, B, c->ws.Q, va, vb, &val, c->kp_max, s, stage == PNP_CRF_PROBE_REVERSE, stage == PNP_CRF_PROBE_SPLAT));
    if (stage == PNP_CRF_PROBE_SLICE) {
        CK(c, crf_slice_add(*L, desc, 0, B, val, norm, c->ws.Q, true, s));
        return crf_emit_q(c, d_out, s);
    }
    hipLaunchKernelGGL(crf_probe_rows_kernel, dim3(64, B), dim3(256), 0, s, L->idbase, desc, L->which, val, d_out);
    CHIP(c, hipGetLastError());
    return PNP_OK;
}
