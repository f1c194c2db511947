// The stand-alone DenseCRF of include/pnp_hip.h (pnp_crf_create ... pnp_crf_infer): the mean-field of crf.hip on unary energies
// the caller brings, with kernel widths the caller chooses, in a solver that owns its workspace and needs no pnp_engine -- what
// pydensecrf's DenseCRF2D is to the reference (PnP_OVSS_0514_updated_segmentation.py:1063-1073).
//
// Reused as they are (kernels.h): crf_build_lattice, crf_lattice_norm, crf_filter, crf_update and their PostDesc layout -- one
// channel group per row, the whole batch as one chunk, driven exactly as post.hip's crf_iterate drives them.  New here: the
// solver, and the two layout kernels between the caller's channel-major (K, H*W) planes (pydensecrf's layout) and the
// pixel-major Kp-float rows the mean-field kernels work on.  No arithmetic happens in this file: the planes <-> rows kernels
// move floats, and the labels come from the last update's own argmax (CrfLabelOut with an identity table).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/pnp_hip.h"
#include "common.h"
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

}  // namespace pnp

// ------------------------------------------------------------------------------------------ the solver
struct pnp_crf {
    int device = 0;
    // -- fixed by pnp_crf_create
    int maxB = 0, maxK = 0, maxKp = 0, max_pix_img = 0;
    int64_t max_total_pix = 0;
    size_t val_cap = 0, valg_cap = 0;             // floats of the bilateral / Gaussian lattice value buffers
    float *unary = nullptr, *Q = nullptr, *va = nullptr, *vb = nullptr, *vga = nullptr, *vgb = nullptr, *norm[2] = {nullptr, nullptr};
    CrfLattice lat[2]{};                          // [0] Gaussian, [1] bilateral
    CrfBuildScratch scratch{};
    PostDesc* d_desc = nullptr;
    int32_t* d_lut = nullptr;                     // 0 .. 255: the label of a channel is its index
    size_t* d_label_off = nullptr;                // [B] first pixel of every image in the concatenated label output
    std::vector<void*> allocs;
    size_t alloc_bytes = 0;
    // -- the batch of the last pnp_crf_set_batch
    bool ready = false;
    int B = 0, kp_max = 0, maxHW = 0;
    int64_t total_pix = 0;
    std::vector<PostDesc> desc;
    std::vector<size_t> h_label_off;
    std::vector<int> gauss_sig;                   // (H, W) list and ...
    float gauss_xy = 0.f;                         // ... width the Gaussian lattice was last built for
    char err[512] = {0};
};

namespace {

constexpr int CRF_MAX_IMAGES = 64;                // IMG_BITS of the packed lattice key (crf.hip)
constexpr int CRF_MAX_LABELS = 255;               // uint8 labels
// |coordinate| a bilateral lattice key may reach: 11 bits per coordinate less the d + 1 = 6 of the canonical simplex
// (lattice_embed_kernel's range flag)
constexpr int CRF_KEY_LIMIT = (1 << 10) - 6;

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
    if (hipMalloc(&p, bytes) != hipSuccess) return cfail(c, PNP_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    c->allocs.push_back(p);
    c->alloc_bytes += bytes;
    if (zero && hipMemset(p, 0, bytes) != hipSuccess) return cfail(c, PNP_ERR_HIP, "hipMemset failed");
    *out = reinterpret_cast<T*>(p);
    return PNP_OK;
}

// what pnp_post_reserve allocates for the CRF, for one channel group and one chunk = the whole batch
int crf_reserve(pnp_crf* c) {
    const size_t TP = (size_t)c->max_total_pix, Kp = (size_t)c->maxKp, B = (size_t)c->maxB;
    CK(c, calloc_dev(c, &c->d_desc, B));
    CK(c, calloc_dev(c, &c->d_label_off, B + 1));
    CK(c, calloc_dev(c, &c->d_lut, 256));
    {
        int32_t ident[256];
        for (int i = 0; i < 256; i++) ident[i] = i;
        CHIP(c, hipMemcpy(c->d_lut, ident, sizeof(ident), hipMemcpyHostToDevice));
    }
    CK(c, calloc_dev(c, &c->unary, TP * Kp));
    CK(c, calloc_dev(c, &c->Q, TP * Kp));
    CK(c, calloc_dev(c, &c->norm[0], TP));
    CK(c, calloc_dev(c, &c->norm[1], TP));
    for (int t = 0; t < 2; t++) {
        const int D1 = t == 0 ? 3 : 6;
        const size_t cap = TP * D1;
        CrfLattice& L = c->lat[t];
        L.D1 = D1;
        L.which = t;
        L.cap = cap;
        CK(c, calloc_dev(c, &L.bary, cap));
        CK(c, calloc_dev(c, &L.vals, cap));
        CK(c, calloc_dev(c, &L.ent, cap));
        CK(c, calloc_dev(c, &L.offset, cap));
        CK(c, calloc_dev(c, &L.seg_start, cap + 1));
        CK(c, calloc_dev(c, &L.seg_lo, cap));
        CK(c, calloc_dev(c, &L.seg_hi, cap));
        CK(c, calloc_dev(c, &L.ukeys, cap));
        CK(c, calloc_dev(c, &L.idbase, B + 1));
        CK(c, calloc_dev(c, &L.n1, cap * D1));
        CK(c, calloc_dev(c, &L.n2, cap * D1));
        CK(c, calloc_dev(c, &L.nbr8, cap * (D1 / 2)));
    }
    const size_t cap6 = c->lat[1].cap;            // E of CrfBuildScratch (kernels.h)
    CrfBuildScratch& sc = c->scratch;
    CK(c, calloc_dev(c, &sc.keys_a, cap6));
    CK(c, calloc_dev(c, &sc.keys_b, cap6));
    CK(c, calloc_dev(c, &sc.vals_a, cap6));
    CK(c, calloc_dev(c, &sc.head, cap6));
    CK(c, calloc_dev(c, &sc.incl, cap6));
    CK(c, calloc_dev(c, &sc.n1k, cap6 * 6));
    CK(c, calloc_dev(c, &sc.n2k, cap6 * 6));
    CK(c, calloc_dev(c, &sc.range_err, 1, true));
    sc.temp_bytes = crf_sort_temp_bytes(cap6);
    CK(c, calloc_dev(c, &sc.temp, sc.temp_bytes));
    // lattice value buffers: one row of Kp floats per lattice point, at most 6 (bilateral) / 3 (Gaussian) points per pixel;
    // crf_lattice_norm also uses va / vb as scalar scratch of one float per lattice point
    c->val_cap = std::max(TP * 6 * Kp, cap6);
    CK(c, calloc_dev(c, &c->va, c->val_cap));
    CK(c, calloc_dev(c, &c->vb, c->val_cap));
    c->valg_cap = TP * 3 * Kp;
    CK(c, calloc_dev(c, &c->vga, c->valg_cap));
    CK(c, calloc_dev(c, &c->vgb, c->valg_cap));
    return PNP_OK;
}

// Host only: validates the batch against the reserved bounds and lays it out (PostDesc, one channel group per row)
int crf_layout(pnp_crf* c, const pnp_crf_batch* b) {
    const int B = b->B;
    c->desc.assign(B, PostDesc{});
    c->h_label_off.assign(B + 1, 0);
    c->kp_max = c->maxHW = 0;
    size_t off = 0, qoff = 0, v[2] = {0, 0};
    int64_t pix = 0;
    for (int i = 0; i < B; i++) {
        PostDesc d{};
        d.H = b->H[i]; d.W = b->W[i]; d.K = b->K[i];
        if (d.H <= 0 || d.W <= 0) return cfail(c, PNP_ERR_ARG, "image %d: bad size %d x %d", i, d.H, d.W);
        if (d.K < 2 || d.K > c->maxK) return cfail(c, PNP_ERR_ARG, "image %d: %d labels, the solver holds 2..%d", i, d.K, c->maxK);
        const int64_t n = (int64_t)d.H * d.W;
        if (n > c->max_pix_img) return cfail(c, PNP_ERR_ARG, "image %d: %d x %d = %lld pixels, reserved %d per image", i, d.H, d.W, (long long)n, c->max_pix_img);
        d.C = d.K; d.has_bg = 0; d.G = 1; d.Kg = d.K;
        d.Kp = (d.K + 3) / 4 * 4;
        // the iteration kernels address an image's rows with 24-bit ids and 32-bit byte offsets (crf.hip)
        if (n * 6 >= (1 << 24) || n * 6 * d.Kp * 4 >= ((int64_t)1 << 32))
            return cfail(c, PNP_ERR_ARG, "image %d: %lld pixels x %d labels exceed the per-image addressing of the mean-field kernels", i, (long long)n, d.K);
        d.pix0 = (int)pix;
        d.off = off;
        d.qoff = qoff;
        for (int t = 0; t < 2; t++) {
            d.voff[t] = v[t];
            v[t] += (size_t)n * (t == 0 ? 3 : 6) * d.Kp;
        }
        c->desc[i] = d;
        c->h_label_off[i] = (size_t)pix;
        off += (size_t)d.K * n;
        qoff += (size_t)d.Kp * n;
        pix += n;
        c->kp_max = std::max(c->kp_max, d.Kp);
        c->maxHW = std::max(c->maxHW, (int)n);
    }
    c->h_label_off[B] = (size_t)pix;
    if (pix > c->max_total_pix) return cfail(c, PNP_ERR_ARG, "batch has %lld pixels, reserved %lld", (long long)pix, (long long)c->max_total_pix);
    if (v[1] > c->val_cap || v[0] > c->valg_cap) return cfail(c, PNP_ERR_ARG, "batch needs %zu lattice value floats, reserved %zu", v[1], c->val_cap);
    c->B = B;
    c->total_pix = pix;
    return PNP_OK;
}

}  // namespace

extern "C" int pnp_crf_create(int32_t device, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image,
                              int32_t max_labels, pnp_crf** out) {
    if (!out) return PNP_ERR_ARG;
    *out = nullptr;
    if (device < 0 || max_batch < 1 || max_batch > CRF_MAX_IMAGES || max_total_pixels < 1 || max_pixels_per_image < 1 ||
        max_pixels_per_image > max_total_pixels || max_labels < 2 || max_labels > CRF_MAX_LABELS)
        return PNP_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return PNP_ERR_HIP;
    pnp_crf* c = new pnp_crf();
    c->device = device;
    c->maxB = max_batch;
    c->max_total_pix = max_total_pixels;
    c->max_pix_img = max_pixels_per_image;
    c->maxK = max_labels;
    c->maxKp = (max_labels + 3) / 4 * 4;
    *out = c;                                     // handed out on failure too: pnp_crf_last_error says why, pnp_crf_destroy frees
    return crf_reserve(c);
}

extern "C" void pnp_crf_destroy(pnp_crf* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void* p : c->allocs) (void)hipFree(p);
    delete c;
}

extern "C" size_t pnp_crf_allocated_bytes(const pnp_crf* c) { return c ? c->alloc_bytes : 0; }

extern "C" const char* pnp_crf_last_error(const pnp_crf* c) { return c ? c->err : "null solver"; }

extern "C" int pnp_crf_set_batch(pnp_crf* c, const pnp_crf_batch* b, float pos_xy, float bi_xy, float bi_rgb, void* stream) {
    if (!c) return PNP_ERR_ARG;
    c->ready = false;
    if (!c->va || !c->vgb) return cfail(c, PNP_ERR_STATE, "the solver's workspace was not allocated (pnp_crf_create failed)");
    if (!b) return cfail(c, PNP_ERR_ARG, "batch is null");
    if (b->B < 1 || b->B > c->maxB) return cfail(c, PNP_ERR_ARG, "batch of %d images, the solver holds 1..%d", b->B, c->maxB);
    if (!b->H || !b->W || !b->K || !b->d_rgb || !b->d_unary) return cfail(c, PNP_ERR_ARG, "batch has null arrays (H, W, K, d_rgb, d_unary)");
    if (!(pos_xy > 0.f) || !(bi_xy > 0.f) || !(bi_rgb > 0.f))
        return cfail(c, PNP_ERR_ARG, "kernel widths must be positive (pos_xy=%g, bi_xy=%g, bi_rgb=%g)", pos_xy, bi_xy, bi_rgb);
    if (int r = crf_layout(c, b)) return r;
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    const int B = c->B;
    // (pageable host memory: copied into the runtime's staging buffer at enqueue time, so the vectors may be rewritten by the
    // next call without a synchronisation)
    CHIP(c, hipMemcpyAsync(c->d_desc, c->desc.data(), sizeof(PostDesc) * B, hipMemcpyHostToDevice, s));
    CHIP(c, hipMemcpyAsync(c->d_label_off, c->h_label_off.data(), sizeof(size_t) * (B + 1), hipMemcpyHostToDevice, s));
    CK(c, crf_planes_rows(true, c->d_desc, const_cast<float*>(b->d_unary), c->unary, B, c->maxHW, c->kp_max, s));
    // both lattices and their normalisers; the Gaussian (xy-only) one depends on the image sizes and its width alone and is
    // kept across batches.  Each build synchronises once (lattice size + range flag read-back)
    std::vector<int> sig;
    for (const PostDesc& d : c->desc) { sig.push_back(d.H); sig.push_back(d.W); }
    int range_err = 0, points = 0;
    for (int t = 0; t < 2; t++) {
        if (t == 0 && sig == c->gauss_sig && pos_xy == c->gauss_xy) continue;
        if (t == 0) c->gauss_sig.clear();
        const size_t entries = (size_t)c->total_pix * c->lat[t].D1;
        CK(c, crf_build_lattice(c->lat[t].D1 - 1, c->lat[t], c->d_desc, c->desc.data(), b->d_rgb, t == 0 ? pos_xy : bi_xy, bi_rgb, B,
                                entries, c->maxHW, c->scratch, &range_err, &points, s));
        CK(c, crf_lattice_norm(c->lat[t], c->d_desc, B, c->maxHW, entries, c->va, c->vb, c->norm[t], s));
        if (range_err) {                          // leave no stale state behind: the next set_batch rebuilds both lattices
            c->gauss_sig.clear();
            (void)hipMemsetAsync(c->scratch.range_err, 0, sizeof(int), s);
            if (t == 0)
                return cfail(c, PNP_ERR_ARG, "lattice key range exceeded: a Gaussian coordinate leaves the 16-bit key; pos_xy = %g is too small for these images", pos_xy);
            return cfail(c, PNP_ERR_ARG,
                         "lattice key range exceeded: a bilateral coordinate leaves the 11-bit key (|coordinate| must stay below %d); "
                         "bi_rgb = %g (bi_xy = %g) is too small for these images",
                         CRF_KEY_LIMIT, bi_rgb, bi_xy);
        }
        if (t == 0) {
            c->gauss_sig = sig;
            c->gauss_xy = pos_xy;
        }
    }
    c->ready = true;
    return PNP_OK;
}

extern "C" int pnp_crf_infer(pnp_crf* c, int32_t iters, float pos_w, float bi_w, float* d_q, uint8_t* d_labels, void* stream) {
    if (!c) return PNP_ERR_ARG;
    if (iters < 0) return cfail(c, PNP_ERR_ARG, "iters = %d", iters);
    if (!c->ready) return cfail(c, PNP_ERR_STATE, "no batch is set: call pnp_crf_set_batch first (a failed call leaves none)");
    hipStream_t s = (hipStream_t)stream;
    CHIP(c, hipSetDevice(c->device));
    const int B = c->B;
    // labels: the argmax the last update does on the marginals it has just normalised (first maximum, a NaN wins), through
    // the identity table (stride 0: the same table for every image)
    CrfLabelOut lab;
    if (d_labels) {
        lab.lab[0] = d_labels;
        lab.lut = c->d_lut;
        lab.lut_stride = 0;
        lab.label_off = c->d_label_off;
    }
    // as post.hip's crf_iterate: Q0 = softmax(-U), then per iteration both filters and the update
    CK(c, crf_update(c->lat[0], c->lat[1], c->d_desc, 0, B, c->vga, c->va, c->norm[0], c->norm[1], c->unary, c->Q, pos_w, bi_w, 0,
                     c->kp_max, 1, s, iters == 0 ? lab : CrfLabelOut()));
    for (int it = 0; it < iters; it++) {
        const float *rg = nullptr, *rb = nullptr;
        CK(c, crf_filter(c->lat[0], c->d_desc, 0, B, c->Q, c->vga, c->vgb, &rg, c->kp_max, s));
        CK(c, crf_filter(c->lat[1], c->d_desc, 0, B, c->Q, c->va, c->vb, &rb, c->kp_max, s));
        CK(c, crf_update(c->lat[0], c->lat[1], c->d_desc, 0, B, rg, rb, c->norm[0], c->norm[1], c->unary, c->Q, pos_w, bi_w, 1,
                         c->kp_max, 1, s, it == iters - 1 ? lab : CrfLabelOut()));
    }
    if (d_q) CK(c, crf_planes_rows(false, c->d_desc, d_q, c->Q, B, c->maxHW, c->kp_max, s));
    return PNP_OK;
}
