// The reverse mode of the DenseCRF's feature-term mean-field: its kernels and their launchers.  The lattices are those of
// crf_lattice.hip (the algorithm: that file's header), the forward kernels and crf_filter are in crf_meanfield.hip, the shared
// helpers in crf_device.h, the pieces of the tiled kernels -- the forward's -- in crf_tile.h.
#include "crf_tile.h"

namespace pnp {

// ------------------------------------------------------------------------------------------
// Reverse mode of the T-term mean-field (crf_meanfield_backward, pnp_crf_backward_terms).  One update is
//   logit = -U + sum_t C_t (A_t Q),  Q' = softmax(logit),  A_t = alpha N_t S^T B_d .. B_0 S N_t
// (S the splat, B_j one blur axis, N_t the normaliser).  Each B_j is symmetric but their product is not, so the adjoint
// A_t^T = alpha N_t S^T B_0 .. B_d S N_t is the same splat and slice around the blur axes in REVERSE order
// (crf_filter with reverse; densecrf's compute(..., reverse = true)).  Per update, from the cotangent g of Q':
//   dl = Q' (.) (g - <g, Q'>)                          crf_softmax_backward_kernel, which also takes dl off the unary gradient
//   h_t = C_t^T dl                                     crf_term_backward_kernel (and, asked for, the compatibility gradient)
//   g  <- sum_t A_t^T h_t                              crf_filter (reverse) + crf_slice_add_kernel
// No floating-point atomics: every sum has an order that the batch fixes (pixel order inside a tile in fp32, then tiles of an
// image and images of the batch in order in fp64), so two calls give the same bits whatever the grid.

// dl = Q (.) (g - <g, Q>) for every pixel of images img0 + blockIdx.y; gU -= dl.  LPP lanes share a pixel (one 16-byte chunk
// each, LPP the power of two that covers the row: Kp <= 256 keeps it within a wave); the dot product is the lane's four
// products left to right, then an xor butterfly over the group -- the same value in every lane, the same order in every call.
// Pad floats: Q's are zero, so dl's are.
__global__ __launch_bounds__(256) void crf_softmax_backward_kernel(const PostDesc* __restrict__ imgs, const float* __restrict__ Q,
                                                                   const float* __restrict__ g, float* __restrict__ dl,
                                                                   float* __restrict__ gU, int img0) {
    const int b = img0 + blockIdx.y;
    const int n = imgs[b].H * imgs[b].W, K4 = imgs[b].Kp >> 2;
    int sh = 0;
    while ((1 << sh) < K4) sh++;
    const int LPP = 1 << sh, PPB = 256 >> sh;
    const int c = threadIdx.x & (LPP - 1), pl = threadIdx.x >> sh;
    const bool has = c < K4;
    const size_t qoff = imgs[b].qoff;
    const f32x4* const Q4 = reinterpret_cast<const f32x4*>(Q + qoff);
    const f32x4* const G4 = reinterpret_cast<const f32x4*>(g + qoff);
    f32x4* const D4 = reinterpret_cast<f32x4*>(dl + qoff);
    f32x4* const U4 = reinterpret_cast<f32x4*>(gU + qoff);
    for (int p = blockIdx.x * PPB + pl; p < n; p += gridDim.x * PPB) {       // (p is the same in all lanes of a group)
        const size_t at = (size_t)p * K4 + (has ? c : 0);                    // lanes past the row redo chunk 0 and add nothing
        const f32x4 q = Q4[at], gg = G4[at];
        float d = has ? ((q[0] * gg[0] + q[1] * gg[1]) + q[2] * gg[2]) + q[3] * gg[3] : 0.f;
        for (int m = LPP >> 1; m; m >>= 1) d += __shfl_xor(d, m, LPP);
        if (has) {
            f32x4 o, u = U4[at];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                o[i] = q[i] * (gg[i] - d);
                u[i] = u[i] - o[i];
            }
            D4[at] = o;
            U4[at] = u;
        }
    }
}

// One term of the backward update on a TW x TH pixel tile, from the pieces of crf_term_update_kernel (crf_tile.h: tiles, item
// walk, wave roles, LDS-staged slice records, slice, store loop) in the XCD-affine image schedule: h = C^T dl -- w dl
// (KIND 0), wvec (.) dl (1), h[k] = sum_l M[l][k] dl[l] (2: row k of the transposed
// matrix MT is contiguous; lane = pixel, rows through scalar loads as in the forward's phase 2) -- into the rows of `h`.
// val non-null (the forward-filtered values of Q_{i-1}): the tile also slices msg = A Q_{i-1} (crf_gather_rows / crf_slice_rows,
// the forward's bits) and leaves the compatibility gradient of its pixels, in pixel order in fp32, as ONE partial of psz floats at
// part[(tile0[b] - tile0[img0] + tile - t_lo) * psz]: sum_p sum_l dl msg (KIND 0), [l] sum_p dl[l] msg[l] (1), [l * K + k] sum_p dl[l]
// msg[k] (2: a thread owns entries tid, tid + 256, ..; both tiles stay in LDS, rows of Kp + 1 floats).  Pixels of an edge
// tile outside the image carry dl = 0.  crf_grad_reduce adds the partials.
template <int D1, int KIND>
__global__ __launch_bounds__(256) void crf_term_backward_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs, const float* __restrict__ val,
                                                                const float* __restrict__ norm, const float* __restrict__ dl,
                                                                float* __restrict__ h, float w, const float* __restrict__ wvec,
                                                                const float* __restrict__ MT, int ldm, float alpha, int img0, int nimg, int TP,
                                                                float* __restrict__ part, const int* __restrict__ tile0, int psz, int t_lo,
                                                                int t_hi) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // dl [TP][Kp + 1], msg / h [TP][Kp + 1], the slice records
    __shared__ float red[256];                                          // (KIND 0: the per-label sums of a tile)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int tid = threadIdx.x;
    const int TW = crf_tile_w(TP), TH = TP / TW;
    const int tw_shift = __ffs(TW) - 1;
    const CrfWaveRole wr = crf_wave_role(TP, tid);                      // (KIND 2)
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int b, part_i, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part_i, parts); wi++) {
        const PostDesc im = imgs[b];
        const int K = im.K, Kp = im.Kp, K4 = Kp >> 2, ldt = Kp + 1;
        const int lo = L.idbase[b];
        const CrfTiles tiles = crf_tiles(im, TW, TH);
        // the launch takes tiles [t_lo, t_hi) of every image (all of them, or a span of one image whose partials fill the
        // buffer), so the slice's share is taken of that window
        const int ntiles = tiles.ntiles;
        const int tl0 = t_lo < ntiles ? t_lo : ntiles, nt = (t_hi < ntiles ? t_hi : ntiles) - tl0;
        const CrfShare sh = crf_share(nt, part_i, parts);
        const int tfirst = tl0 + sh.first, tend = tl0 + sh.end;
        const char* const Db = reinterpret_cast<const char*>(dl + im.qoff);
        const char* const Vb = reinterpret_cast<const char*>(val ? val + im.voff[0] : nullptr);
        f32x4* const H4 = reinterpret_cast<f32x4*>(h + im.qoff);
        const uint32_t rowb = (uint32_t)K4 * 16u;
        float* const msg = tile + TP * ldt;
        int* const rec_o = reinterpret_cast<int*>(tile + 2 * TP * ldt);
        float* const rec_w = reinterpret_cast<float*>(rec_o + TP * D1);
        float* const rec_n = rec_w + TP * D1;
        const int tbase = val ? tile0[b] - tile0[img0] - tl0 : 0;
        const CrfItemWalk it0(tid, K4);
        for (int tl = tfirst + slot; tl < tend; tl += bpx) {
            const CrfTileAt at = tiles.at(tl, TW, TH, tw_shift, im);
            if (val) {
                for (int pl = tid; pl < TP; pl += 256) {                 // slice records, one pixel per thread
                    const size_t g = (size_t)im.pix0 + at.pixel_of(pl);
                    crf_stage_record<D1>(L, lo, g, pl, rec_o, rec_w);
                    rec_n[pl] = norm[g];
                }
                __syncthreads();
            }
            // phase 1: the dl chunk of every (pixel, chunk) item, its message chunk if asked for, and h without a matrix
            for (CrfItemWalk it = it0; it.item < TP * K4; it.next()) {
                const int pl = it.pl, c = it.c, px = at.pixel_of(pl);
                const bool in = at.inside(pl);
                const uint32_t cofs = (uint32_t)c * 16u;
                const f32x4 d = in ? *reinterpret_cast<const f32x4*>(Db + (__umul24((uint32_t)px, rowb) + cofs)) : zero;
                if (val) {
                    f32x4 vv[D1];
                    crf_gather_rows<D1>(Vb, rec_o + pl * D1, rowb, cofs, vv);
                    const f32x4 o = crf_slice_rows<D1>(vv, rec_w + pl * D1, alpha);
                    const float nr = rec_n[pl];
#pragma unroll
                    for (int i = 0; i < 4; i++) msg[pl * ldt + 4 * c + i] = __fmul_rn(o[i], nr);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) tile[pl * ldt + 4 * c + i] = d[i];
                if (KIND != 2 && in) {
                    f32x4 wl = {w, w, w, w};
                    if (KIND == 1) wl = *reinterpret_cast<const f32x4*>(wvec + 4 * c);
                    f32x4 hh;
#pragma unroll
                    for (int i = 0; i < 4; i++) hh[i] = wl[i] * d[i];
                    H4[(size_t)px * K4 + c] = hh;
                }
            }
            __syncthreads();
            if (val) {   // the tile's compatibility gradient: fixed entries per thread, pixels ascending
                float* const P = part + (size_t)(tbase + tl) * psz;
                if (KIND == 2) {
                    for (int e = tid; e < K * K; e += 256) {
                        const int l = e / K, k = e - l * K;
                        const float* a = tile + l;
                        const float* m = msg + k;
                        float acc = 0.f;
                        for (int p = 0; p < TP; p++) acc += a[p * ldt] * m[p * ldt];
                        P[e] = acc;
                    }
                } else {
                    for (int l = tid; l < K; l += 256) {
                        float acc = 0.f;
                        for (int p = 0; p < TP; p++) acc += tile[p * ldt + l] * msg[p * ldt + l];
                        if (KIND == 1) P[l] = acc;
                        else red[l] = acc;
                    }
                    if (KIND == 0) {
                        __syncthreads();
                        if (tid == 0) {
                            float acc = 0.f;
                            for (int l = 0; l < K; l++) acc += red[l];
                            P[0] = acc;
                        }
                    }
                }
                __syncthreads();
            }
            if (KIND == 2) {   // h[k] = sum_l M[l][k] dl[l] into the message tile (its last reader is behind the barrier above)
                const float* const x = tile + wr.pxc * ldt;
                for (int k0 = wr.lg * CRF_CL; k0 < K; k0 += wr.NG * CRF_CL) {
                    float a[CRF_CL];
#pragma unroll
                    for (int i = 0; i < CRF_CL; i++) a[i] = 0.f;
                    const float* tm = MT + (size_t)k0 * ldm;             // (rows past K: the zero pad of the transposed matrix)
#pragma unroll 4
                    for (int l = 0; l < K; l++) {
                        const float dv = x[l];
#pragma unroll
                        for (int i = 0; i < CRF_CL; i++) a[i] += tm[i * ldm + l] * dv;
                    }
#pragma unroll
                    for (int i = 0; i < CRF_CL; i++)
                        if (wr.act && k0 + i < Kp) msg[wr.px2 * ldt + k0 + i] = a[i];
                }
                __syncthreads();
                crf_store_tile<false>(msg, ldt, at, it0, TP, H4);
                __syncthreads();
            }
        }
    }
}

// The partials of crf_term_backward_kernel in fp64, in an order the batch fixes.  Stage 1: one thread per (image of the span,
// entry) adds that image's tiles [t_lo, t_hi) in order, onto the image's sum so far if t_lo > 0.  Stage 2: one thread per entry
// adds the images of the span in order onto the running sum acc[entry], which the caller carries over spans and iterations --
// so cutting a batch into spans of images, or one image into spans of tiles, moves no bit.
__global__ __launch_bounds__(256) void crf_grad_image_kernel(const float* __restrict__ part, const int* __restrict__ tile0, int img0, int psz,
                                                             double* __restrict__ img_sum, int t_lo, int t_hi) {
    const int b = img0 + blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= psz) return;
    const int ntiles = tile0[b + 1] - tile0[b];
    const int tl0 = t_lo < ntiles ? t_lo : ntiles;
    const int t0 = tile0[b] - tile0[img0], t1 = t0 + (t_hi < ntiles ? t_hi : ntiles) - tl0;
    const float* p = part + (size_t)t0 * psz + e;
    double s = t_lo > 0 ? img_sum[(size_t)blockIdx.y * psz + e] : 0.0;
    int t = t0;
    for (; t + 4 <= t1; t += 4, p += (size_t)4 * psz) {
        const float v0 = p[0], v1 = p[psz], v2 = p[(size_t)2 * psz], v3 = p[(size_t)3 * psz];
        s += (double)v0;
        s += (double)v1;
        s += (double)v2;
        s += (double)v3;
    }
    for (; t < t1; t++, p += psz) s += (double)*p;
    img_sum[(size_t)blockIdx.y * psz + e] = s;
}
__global__ __launch_bounds__(256) void crf_grad_final_kernel(const double* __restrict__ img_sum, int nimg, int psz, double* __restrict__ acc) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= psz) return;
    double s = acc[e];
    for (int i = 0; i < nimg; i++) s += img_sum[(size_t)i * psz + e];
    acc[e] = s;
}
__global__ __launch_bounds__(256) void crf_grad_emit_kernel(const double* __restrict__ acc, int n, float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = (float)acc[e];
}

// g[p] (+)= norm[p] * alpha * sum_v bary_v val_v: the slice of A^T h into the cotangent rows -- a store for the first term of
// an update, a read-modify-write after it.  (pixel, 16-byte chunk) items over 16 x 16 pixel tiles in the XCD-affine schedule,
// sliced with the forward's pieces (crf_tile.h); no LDS: the D1 vertex ids and weights of a pixel are read by each of its lanes
// (one cached line per pixel), and pixels outside the image are skipped.
template <int D1>
__global__ __launch_bounds__(256) void crf_slice_add_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs, const float* __restrict__ val,
                                                            const float* __restrict__ norm, float* __restrict__ g, int first, float alpha,
                                                            int img0, int nimg) {
    constexpr int TW_SHIFT = 4, TW = 1 << TW_SHIFT, TH = 16, TP = TW * TH;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int tid = threadIdx.x;
    int b, part_i, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part_i, parts); wi++) {
        const PostDesc im = imgs[b];
        const int K4 = im.Kp >> 2;
        const int lo = L.idbase[b];
        const CrfTiles tiles = crf_tiles(im, TW, TH);
        const CrfShare sh = crf_share(tiles.ntiles, part_i, parts);
        const char* const Vb = reinterpret_cast<const char*>(val + im.voff[0]);
        f32x4* const G4 = reinterpret_cast<f32x4*>(g + im.qoff);
        const uint32_t rowb = (uint32_t)K4 * 16u;
        const CrfItemWalk it0(tid, K4);
        for (int tl = sh.first + slot; tl < sh.end; tl += bpx) {
            const CrfTileAt at = tiles.at(tl, TW, TH, TW_SHIFT, im);
            for (CrfItemWalk it = it0; it.item < TP * K4; it.next()) {
                if (at.inside(it.pl)) {
                    const int px = at.pixel_inside(it.pl);
                    const size_t gi = (size_t)im.pix0 + px;
                    const uint32_t cofs = (uint32_t)it.c * 16u;
                    int ids[D1];
                    float wv[D1];
#pragma unroll
                    for (int v = 0; v < D1; v++) {
                        ids[v] = L.offset[gi * D1 + v] - lo;
                        wv[v] = L.bary[gi * D1 + v];
                    }
                    const float nr = norm[gi];
                    f32x4 vv[D1];
                    crf_gather_rows<D1>(Vb, ids, rowb, cofs, vv);
                    const f32x4 o = crf_slice_rows<D1>(vv, wv, alpha);
                    f32x4* const to = G4 + (size_t)px * K4 + it.c;
                    f32x4 r = {0.f, 0.f, 0.f, 0.f};
                    if (!first) r = *to;
#pragma unroll
                    for (int i = 0; i < 4; i++) r[i] = __fadd_rn(r[i], __fmul_rn(o[i], nr));
                    *to = r;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ host
int crf_softmax_backward(const PostDesc* d_imgs, int img0, int nimg, const float* Q, const float* g, float* dl, float* gU, int max_pixels,
                         int max_kp, hipStream_t s) {
    if (max_kp < 4 || max_kp > 256) return PNP_ERR_ARG;
    int lpp = 1;
    while (lpp < max_kp / 4) lpp <<= 1;
    const int blocks = (max_pixels + 256 / lpp - 1) / (256 / lpp);
    hipLaunchKernelGGL(crf_softmax_backward_kernel, dim3(blocks < 4096 ? blocks : 4096, nimg), dim3(256), 0, s, d_imgs, Q, g, dl, gU, img0);
    return ok();
}

// Pixels per tile of crf_term_backward_kernel for rows of up to max_kp floats and its LDS bytes: crf_term_tile_pixels' rule for
// two tiles and the records of the widest term, so that the tiles of a batch -- and with them the order of its sums -- do
// not depend on the term
int crf_backward_tile_pixels(int max_kp, size_t* smem) { return crf_term_tile_pixels(max_kp, 7, 2, smem); }
int crf_backward_tiles(int H, int W, int tp) {
    const int tw = crf_tile_w(tp), th = tp / tw;
    return ((W + tw - 1) / tw) * ((H + th - 1) / th);
}

int crf_term_backward(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* val, const float* norm, const float* dl,
                      float* h, float w, const float* wvec, const float* MT, int ldm, int max_kp, float* part, const int* tile0, int psz,
                      int t_lo, int t_hi, hipStream_t s) {
    if (max_kp < 4 || max_kp > 256 || ((MT || wvec) && (ldm < max_kp || ldm % CRF_CL != 0))) return PNP_ERR_ARG;
    if (val && (!part || !tile0 || psz < 1)) return PNP_ERR_ARG;
    if (t_lo < 0 || t_hi <= t_lo || (t_lo > 0 && nimg != 1)) return PNP_ERR_ARG;
    size_t smem = 0;
    const int tp = crf_backward_tile_pixels(max_kp, &smem);
    return crf_dispatch<2, 7>(L.D1, [&](auto d1) {
        constexpr int D1 = decltype(d1)::value;              // (kernel KIND 2: matrix, 1: vector, 0: scalar weight)
        return crf_launch_tiled(MT ? crf_term_backward_kernel<D1, 2> : wvec ? crf_term_backward_kernel<D1, 1> : crf_term_backward_kernel<D1, 0>,
                                smem, s, L, d_imgs, val, norm, dl, h, w, wvec, MT, ldm, crf_alpha(D1 - 1), img0, nimg, tp, part, tile0, psz, t_lo,
                                t_hi);
    });
}

int crf_grad_reduce(const float* part, const int* tile0, int img0, int nimg, int psz, double* img_sum, double* acc, int t_lo, int t_hi,
                    bool done, hipStream_t s) {
    const int blocks = (psz + 255) / 256;
    hipLaunchKernelGGL(crf_grad_image_kernel, dim3(blocks, nimg), dim3(256), 0, s, part, tile0, img0, psz, img_sum, t_lo, t_hi);
    if (done) hipLaunchKernelGGL(crf_grad_final_kernel, dim3(blocks), dim3(256), 0, s, img_sum, nimg, psz, acc);
    return ok();
}

int crf_grad_emit(const double* acc, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(crf_grad_emit_kernel, dim3((n + 255) / 256), dim3(256), 0, s, acc, n, out);
    return ok();
}

int crf_slice_add(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* val, const float* norm, float* g, bool first,
                  hipStream_t s) {
    return crf_dispatch<2, 7>(L.D1, [&](auto d1) {
        constexpr int D1 = decltype(d1)::value;
        static PerDeviceInt g_;                              // per instantiation and device ordinal (common.h)
        const int nb = g_.get([] { return resident_grid(crf_slice_add_kernel<D1>, 256, 0); });
        hipLaunchKernelGGL((crf_slice_add_kernel<D1>), dim3(nb), dim3(256), 0, s, L, d_imgs, val, norm, g, first ? 1 : 0, crf_alpha(D1 - 1), img0,
                           nimg);
        return ok();
    });
}

}  // namespace pnp
