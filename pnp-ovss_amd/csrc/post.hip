// The post-processing entry points of include/pnp_hip.h (pnp_post_reserve ... pnp_postprocess_pair): token merge, threshold,
// upsample, blur and DenseCRF of a batch of differently sized images.  Host logic only: the kernels are in
// pipeline_kernels.hip, crf_lattice.hip, crf_meanfield.hip and sort.hip; the state is pnp_engine::Post (engine.h).  The DenseCRF arrays, lattice build and
// mean-field sequence are crf_solver.h's, shared with the stand-alone solver (crf_op.hip); the engine's own are the chunking, the
// paired two-group layout, the stage profile and the reference's fixed parameters.
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.h"

using namespace pnp;

namespace {

// The reference's DenseCRF (PnP.py:1036-1041): 10 mean-field iterations, a Gaussian pairwise term of weight 7 with sxy = 3 and a
// bilateral one of weight 10 with sxy = 50, srgb = 5.  The lattices are built for these sigmas; pnp_densecrf refuses others.
constexpr int CRF_ITERS = 10;
constexpr float CRF_POS_W = 7.0f, CRF_POS_XY = 3.0f, CRF_BI_W = 10.0f, CRF_BI_XY = 50.0f, CRF_BI_RGB = 5.0f;

}  // namespace

extern "C" int pnp_post_reserve(pnp_engine* e, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image,
                                int32_t max_channels, int32_t crf_chunk) {
    if (!e) return PNP_ERR_ARG;
    if (e->post.reserved) return fail(e, PNP_ERR_STATE, "post-process workspace already reserved");
    if (max_batch <= 0 || max_batch > CRF_MAX_IMAGES || max_total_pixels <= 0 || max_pixels_per_image <= 0 || max_channels <= 0 ||
        max_channels > CRF_MAX_LABELS)
        return fail(e, PNP_ERR_ARG, "bad post-process bounds (at most %d images per batch, %d channels)", CRF_MAX_IMAGES, CRF_MAX_LABELS);
    HIPCHK(e, hipSetDevice(e->c.device));
    auto& p = e->post;
    p.maxB = max_batch;
    p.max_total_pix = max_total_pixels;
    p.max_pix_img = max_pixels_per_image;
    p.maxK = max_channels;
    p.chunk = crf_chunk > 0 ? crf_chunk : max_batch;
    const size_t TP = (size_t)max_total_pixels, K = max_channels, B = max_batch;
    for (int g = 0; g < 2; g++) {
        PostDesc* d = nullptr;
        KCHK(e, dalloc(e, &d, B));
        p.view[g] = CrfSpan{d, 0, 0, 0, g + 1};
    }
    KCHK(e, dalloc(e, &p.d_img_cls_off, B + 1));
    p.cls_cap = (int)(B * K + 1);
    p.tok_cap = (int)(B * e->c.max_text_len + 1);
    KCHK(e, dalloc(e, &p.d_cls_off, p.cls_cap + 1));
    KCHK(e, dalloc(e, &p.d_cls_div, p.cls_cap));
    KCHK(e, dalloc(e, &p.d_tok_idx, p.tok_cap));
    p.lut_cap = (int)(B * (K + 1));
    KCHK(e, dalloc(e, &p.d_lut, p.lut_cap));
    KCHK(e, dalloc(e, &p.d_label_off, B + 1));
    p.wts_cap = (int)(B * 4096);
    KCHK(e, dalloc(e, &p.d_wts, p.wts_cap));
    KCHK(e, dalloc(e, &p.d_wt_off, B + 1));
    KCHK(e, dalloc(e, &p.merged, B * K * e->PP));
    KCHK(e, dalloc(e, &p.thr, B * K * e->PP));
    KCHK(e, dalloc(e, &p.maps, TP * K));
    KCHK(e, dalloc(e, &p.maps2, TP * K));
    KCHK(e, dalloc(e, &p.maps3, TP * K));
    KCHK(e, dalloc(e, &p.stats, B * K * 2));
    // CRF
    p.maxKp = crf_row_stride(1, max_channels);
    const size_t Kp = (size_t)p.maxKp;
    // lattice value buffers hold the images of one chunk
    const size_t chunk_pix = (size_t)std::min<int64_t>((int64_t)p.chunk * max_pixels_per_image, max_total_pixels);
    // the paired 1-drop | N-drop run keeps two channel groups per row: size the CRF arrays for it unless that would
    // take more than a third of the free device memory (many classes x large images); pnp_postprocess_pair then runs
    // the two branches one after the other
    {
        const size_t single = (2 * TP * Kp + 2 * chunk_pix * 6 * Kp + 2 * chunk_pix * 3 * Kp) * sizeof(float);
        // ... of what the device has free right now (the rest of this function needs about as much again for maps and lattices)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)96 << 30;
        p.groups_cap = 2 * single <= free_b / 3 ? 2 : 1;
    }
    for (const CrfAlloc& a : crf_reserve_plan(p.crf, B, TP, chunk_pix, Kp, (size_t)p.groups_cap))
        KCHK(e, dalloc(e, reinterpret_cast<char**>(a.dst), a.bytes, a.zero));
    p.reserved = true;
    return PNP_OK;
}

// ------------------------------------------------------------------------------------------ prepare

// scipy _gaussian_kernel1d(sigma = 0.05 * max(H, W)), truncate 4.0  (PnP.py:1150, scale=0.05): appends the radius + 1 weights
// at distance 0 .. radius (w[-j] == w[j])
static void gaussian_taps(int H, int W, std::vector<double>& wts) {
    const double sigma = 0.05 * (double)std::max(H, W);
    const int radius = (int)(4.0 * sigma + 0.5);
    std::vector<double> phi(2 * radius + 1);
    double sum = 0;
    for (int x = -radius; x <= radius; x++) {
        phi[x + radius] = std::exp(-0.5 / (sigma * sigma) * (double)(x * x));
        sum += phi[x + radius];
    }
    for (int j = 0; j <= radius; j++) wts.push_back(phi[radius - j] / sum);
}

// Step 1, host only: validates the batch against the reserved bounds and lays it out -- both descriptor sets, the label and
// blur-tap tables, the batch maxima.  Nothing is enqueued, so an error leaves the stream untouched.
static int post_layout(pnp_engine* e, const pnp_post_batch* b, bool want_crf) {
    auto& p = e->post;
    const int B = b->B;
    const bool own_taps = b->blur_wts && b->blur_wt_off;
    for (auto& d : p.desc) d.assign(B, PostDesc{});
    p.h_label_off.assign(B + 1, 0);
    p.h_wt_off.assign(B + 1, 0);
    p.h_wts.clear();
    p.Cmax = p.Kmax = p.maxHW = p.maxH = p.maxW = p.max_radius = 0;
    p.view[0].kp_max = p.view[1].kp_max = 0;
    CrfOffsets at[2];                          // [layout]; the value offsets are those inside the current CRF chunk (upper bound: entries * Kp)
    size_t chunk_need = 0;                     // bilateral value floats of the first chunk that exceeds what is reserved (0: none)
    for (int i = 0; i < B; i++) {
        PostDesc d{};
        d.H = b->H[i]; d.W = b->W[i]; d.C = b->n_classes[i]; d.has_bg = b->has_bg[i] ? 1 : 0; d.K = d.C + d.has_bg;
        if (d.H <= 0 || d.W <= 0 || d.C <= 0 || d.K > p.maxK) return fail(e, PNP_ERR_ARG, "image %d: bad H/W/classes (K=%d max %d)", i, d.K, p.maxK);
        if ((int64_t)d.H * d.W > p.max_pix_img) return fail(e, PNP_ERR_ARG, "image %d: %dx%d exceeds max_pixels_per_image", i, d.H, d.W);
        if (b->img_cls_off[i + 1] - b->img_cls_off[i] != d.C) return fail(e, PNP_ERR_ARG, "image %d: merge plan has %d classes, expected %d", i, b->img_cls_off[i + 1] - b->img_cls_off[i], d.C);
        d.Kg = d.K;
        for (int g = 0; g < 2; g++) {          // one channel group per row | the paired run's two, packed back to back
            if (i % p.chunk == 0) at[g].voff[0] = at[g].voff[1] = 0;
            // refused with the widest row this engine would run the image with: the paired layout where it is reserved
            if (!crf_layout_image(d, g + 1, at[g]) && want_crf && g < p.groups_cap)
                return fail(e, PNP_ERR_ARG, "image %d: %d x %d pixels x %d floats per row exceed the per-image addressing of the mean-field "
                            "kernels: its DenseCRF cannot be computed", i, d.H, d.W, d.Kp);
            p.desc[g][i] = d;
            p.view[g].kp_max = std::max(p.view[g].kp_max, d.Kp);
        }
        const bool chunk_ends = i + 1 == B || (i + 1) % p.chunk == 0;
        if (chunk_ends && !chunk_need && (p.groups_cap * at[0].voff[1] > p.crf.val_cap || p.groups_cap * at[0].voff[0] > p.crf.valg_cap))
            chunk_need = p.groups_cap * at[0].voff[1];                     // incl. room for the paired run
        p.h_label_off[i] = (size_t)d.pix0;
        p.maxH = std::max(p.maxH, d.H); p.maxW = std::max(p.maxW, d.W); p.maxHW = std::max(p.maxHW, d.H * d.W);
        p.Cmax = std::max(p.Cmax, d.C); p.Kmax = std::max(p.Kmax, d.K);
        p.h_wt_off[i] = (int32_t)p.h_wts.size();
        if (own_taps) {
            for (int j = b->blur_wt_off[i]; j < b->blur_wt_off[i + 1]; j++) p.h_wts.push_back(b->blur_wts[j]);
        } else {
            gaussian_taps(d.H, d.W, p.h_wts);
        }
        p.max_radius = std::max(p.max_radius, (int)p.h_wts.size() - p.h_wt_off[i] - 1);
    }
    p.h_wt_off[B] = (int32_t)p.h_wts.size();
    p.h_label_off[B] = (size_t)at[0].pix;
    if (at[0].pix > p.max_total_pix) return fail(e, PNP_ERR_ARG, "batch has %lld pixels, reserved %lld", (long long)at[0].pix, (long long)p.max_total_pix);
    if ((int)p.h_wts.size() > p.wts_cap) return fail(e, PNP_ERR_ARG, "blur taps exceed reserved capacity");
    const int ncls = b->img_cls_off[B], ntok = b->cls_off[ncls];
    if (ncls > p.cls_cap || ntok > p.tok_cap) return fail(e, PNP_ERR_ARG, "merge plan exceeds reserved capacity");
    if (b->lut_stride < p.Kmax || B * b->lut_stride > p.lut_cap) return fail(e, PNP_ERR_ARG, "bad lut_stride");
    if (chunk_need) return fail(e, PNP_ERR_ARG, "CRF chunk needs %zu value floats, reserved %zu", chunk_need, p.crf.val_cap);
    p.B = B;
    p.lut_stride = b->lut_stride;
    p.d_rgb = b->d_rgb;
    p.d_gt = b->d_gt;
    return PNP_OK;
}

// Step 2: the descriptors and the small tables to the device.  The copies read caller / engine host memory asynchronously:
// pnp_post_prepare's one synchronisation is behind them.
static int post_upload(pnp_engine* e, const pnp_post_batch* b, hipStream_t s) {
    auto& p = e->post;
    const int B = p.B;
    const int ncls = b->img_cls_off[B], ntok = b->cls_off[ncls];
    for (int g = 0; g < 2; g++)                // (the one place that writes through a view's descriptor pointer)
        HIPCHK(e, hipMemcpyAsync(const_cast<PostDesc*>(p.view[g].d_desc), p.desc[g].data(), sizeof(PostDesc) * B, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_img_cls_off, b->img_cls_off, 4 * (B + 1), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_cls_off, b->cls_off, 4 * (ncls + 1), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_cls_div, b->cls_div, 4 * std::max(ncls, 1), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_tok_idx, b->tok_idx, 4 * std::max(ntok, 1), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_lut, b->lut, 4 * (size_t)B * b->lut_stride, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_label_off, p.h_label_off.data(), sizeof(size_t) * (B + 1), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_wts, p.h_wts.data(), 8 * p.h_wts.size(), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(p.d_wt_off, p.h_wt_off.data(), 4 * (B + 1), hipMemcpyHostToDevice, s));
    return PNP_OK;
}

// Step 3: the two lattices of the batch and their normalisers, for the reference's widths.  The bilateral one is built every
// time, so every call synchronises once, inside the build's read-back.
static int post_build_lattices(pnp_engine* e, hipStream_t s) {
    auto& p = e->post;
    const float pos_xy[2] = {CRF_POS_XY, CRF_POS_XY}, bi_xy[2] = {CRF_BI_XY, CRF_BI_XY}, bi_rgb[3] = {CRF_BI_RGB, CRF_BI_RGB, CRF_BI_RGB};
    int range_term = -1;
    const int r = crf_build(p.crf, p.view[0].d_desc, p.desc[0].data(), p.B, p.h_label_off[p.B], p.maxHW, p.d_rgb, pos_xy, bi_xy, bi_rgb,
                            &range_term, s);
    if (range_term >= 0) return fail(e, r, "lattice key out of packing range (image too large for the 64-bit key)");
    if (r != PNP_OK) return fail(e, r, "CRF lattice build failed (%d): %s", r, hipGetErrorString(hipGetLastError()));
    p.has_crf = true;
    return PNP_OK;
}

extern "C" int pnp_post_prepare(pnp_engine* e, const pnp_post_batch* b, int32_t want_crf, void* stream) {
    if (!e || !b) return PNP_ERR_ARG;
    auto& p = e->post;
    if (!p.reserved) return fail(e, PNP_ERR_STATE, "call pnp_post_reserve first");
    if (b->B <= 0 || b->B > p.maxB) return fail(e, PNP_ERR_ARG, "post batch %d out of range", b->B);
    if (!b->H || !b->W || !b->n_classes || !b->has_bg || !b->img_cls_off || !b->cls_off || !b->tok_idx || !b->cls_div || !b->lut)
        return fail(e, PNP_ERR_ARG, "post batch has null tables");
    if (want_crf && !b->d_rgb) return fail(e, PNP_ERR_ARG, "CRF needs d_rgb");
    hipStream_t s = (hipStream_t)stream;
    p.prepared = false;
    if (int r = post_layout(e, b, want_crf != 0)) return r;
    if (int r = post_upload(e, b, s)) return r;
    p.has_crf = false;
    // one synchronisation per batch: the lattice build's, or without a lattice to build this one
    if (want_crf) {
        if (int r = post_build_lattices(e, s)) return r;
    } else {
        HIPCHK(e, hipStreamSynchronize(s));
    }
    p.prepared = true;
    return PNP_OK;
}

// ------------------------------------------------------------------------------------------ stages

#define POST_READY(e)                                                                     \
    if (!(e)) return PNP_ERR_ARG;                                                         \
    if (!(e)->post.prepared) return fail(e, PNP_ERR_STATE, "call pnp_post_prepare first");

extern "C" int pnp_merge_tokens(pnp_engine* e, const float* d_gradcam, int32_t T, void* stream) {
    POST_READY(e);
    auto& p = e->post;
    if (!d_gradcam || T < 5) return fail(e, PNP_ERR_ARG, "bad gradcam / T");
    KCHK(e, merge_tokens(d_gradcam, p.d_cls_off, p.d_tok_idx, p.d_cls_div, p.d_img_cls_off, p.merged, p.B, T, e->PP, p.Cmax,
                         (hipStream_t)stream));
    return PNP_OK;
}

extern "C" int pnp_threshold_upsample(pnp_engine* e, float threshold, int32_t scale01, void* stream) {
    POST_READY(e);
    auto& p = e->post;
    const PostDesc* desc = p.view[0].d_desc;
    hipStream_t s = (hipStream_t)stream;
    KCHK(e, threshold_maps(p.merged, p.d_img_cls_off, p.thr, threshold, p.B, e->PP, p.Cmax, s));
    KCHK(e, upsample_maps(p.thr, desc, p.maps, p.B, e->P, p.Cmax, p.maxHW, s));
    if (scale01) KCHK(e, minmax_normalize(p.maps, desc, p.stats, p.B, p.Cmax, p.maxHW, 1, s));
    KCHK(e, background_channel(p.maps, desc, p.B, p.maxHW, s));
    p.maps_in_2 = false;
    return PNP_OK;
}

extern "C" int pnp_blur_minmax(pnp_engine* e, void* stream) {
    POST_READY(e);
    auto& p = e->post;
    const PostDesc* desc = p.view[0].d_desc;
    hipStream_t s = (hipStream_t)stream;
    KCHK(e, blur_maps(p.maps, p.maps3, p.maps2, desc, p.d_wts, p.d_wt_off, p.B, p.Kmax, p.maxH, p.maxW, p.max_radius, s));
    KCHK(e, minmax_normalize(p.maps2, desc, p.stats, p.B, p.Kmax, p.maxHW, 0, s));
    p.maps_in_2 = true;
    return PNP_OK;
}

// Event bracket of the timed stage (pnp_profile_enable): crf_timer_start records the start event of a run, creating the pair on
// first use, and says whether this run is timed; crf_timer_stop records its end and counts it.
static int crf_timer_start(pnp_engine* e, hipStream_t s, bool* timed) {
    auto& pf = e->crf_prof;
    *timed = pf.on && pf.used < 4096;
    if (!*timed) return PNP_OK;
    if ((int)pf.ev0.size() <= pf.used) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(e, PNP_ERR_HIP, "hipEventCreate failed");
        pf.ev0.push_back(a);
        pf.ev1.push_back(b);
    }
    (void)hipEventRecord(pf.ev0[pf.used], s);
    return PNP_OK;
}
static void crf_timer_stop(pnp_engine* e, hipStream_t s) {
    auto& pf = e->crf_prof;
    (void)hipEventRecord(pf.ev1[pf.used], s);
    pf.used++;
    pf.launches++;
}

// `work` = SURVEY.md 8d, nothing else: per mean-field iteration splat + slice of (3 + 6) simplex vertices per pixel and
// channel, each a 4-byte read or write, plus Q read and written once: (2 * 9 + 2) * K * H * W * 4 bytes.  The term that grows
// with the lattice instead of the pixels is kept BESIDE it (`lattice`, stage 2 of pnp_profile_read_stage): the axis blurs
// read and write the value array of every lattice point (M_g + M_b points of K floats) once per PASS of two axes -- 2 passes
// for the Gaussian lattice (d + 1 = 3 axes), 3 for the bilateral one (6 axes).  Neither figure is what the HBM counters
// see (part of both is served by L2: the kernels are gather-bound)
static void crf_count_bytes(pnp_engine* e, int groups, int iters) {
    const auto& p = e->post;
    double kpix = 0, pix = 0;
    for (const PostDesc& d : p.desc[0]) {
        kpix += (double)d.K * d.H * d.W;
        pix += (double)d.H * d.W;
    }
    const double kavg = pix > 0 ? kpix / pix : 0;
    e->crf_prof.work += (double)iters * 20.0 * 4.0 * groups * kpix;
    e->crf_prof.lattice += (double)iters * 2.0 * 4.0 * groups * kavg * (2.0 * p.crf.lat_points[0] + 3.0 * p.crf.lat_points[1]);
}

// mean-field iterations over the unary rows already in p.crf.unary, chunk by chunk, in the single- or two-group layout `v`.
// labels: when set, the last update of every chunk also writes the label maps (argmax + LUT fused into it: no separate pass over Q)
static int crf_iterate(pnp_engine* e, CrfSpan v, int32_t iters, float pos_w, float bi_w, hipStream_t s,
                       const CrfLabelOut& labels = CrfLabelOut()) {
    auto& p = e->post;
    bool timed = false;
    if (int r = crf_timer_start(e, s, &timed)) return r;
    for (int c0 = 0; c0 < p.B; c0 += p.chunk) {
        v.img0 = c0;
        v.nimg = std::min(p.chunk, p.B - c0);
        KCHK(e, crf_meanfield_start(p.crf, v, s, iters == 0 ? labels : CrfLabelOut()));
        KCHK(e, crf_meanfield(p.crf, v, iters, CrfPairRun{pos_w, bi_w, nullptr, nullptr, 0}, s, labels));
    }
    if (timed) {
        crf_timer_stop(e, s);
        crf_count_bytes(e, v.groups, iters);
    }
    return PNP_OK;
}

extern "C" int pnp_densecrf(pnp_engine* e, int32_t iters, float pos_w, float pos_xy, float bi_w, float bi_xy, float bi_rgb,
                            void* stream) {
    POST_READY(e);
    auto& p = e->post;
    if (!p.has_crf) return fail(e, PNP_ERR_STATE, "batch was prepared without CRF lattices");
    if (pos_xy != CRF_POS_XY || bi_xy != CRF_BI_XY || bi_rgb != CRF_BI_RGB)
        return fail(e, PNP_ERR_ARG, "lattices are built for sxy=%g / sxy=%g, srgb=%g (PnP.py:1036-1041)", CRF_POS_XY, CRF_BI_XY, CRF_BI_RGB);
    hipStream_t s = (hipStream_t)stream;
    const float* maps = p.maps_in_2 ? p.maps2 : p.maps;
    KCHK(e, unary_from_maps(maps, p.view[0].d_desc, p.crf.unary, p.B, p.maxHW, p.maxKp, 0, s));
    return crf_iterate(e, p.view[0], iters, pos_w, bi_w, s);
}

extern "C" int pnp_remap_hist(pnp_engine* e, int32_t from_crf, uint8_t* d_labels, unsigned long long* d_hist, int32_t n_class,
                              void* stream) {
    POST_READY(e);
    auto& p = e->post;
    const PostDesc* desc = p.view[0].d_desc;
    if (!d_labels) return fail(e, PNP_ERR_ARG, "d_labels is null");
    hipStream_t s = (hipStream_t)stream;
    const float* src = from_crf ? p.crf.Q : (p.maps_in_2 ? p.maps2 : p.maps);
    KCHK(e, argmax_remap(src, desc, p.d_lut, p.lut_stride, d_labels, p.d_label_off, from_crf ? 1 : 0, 0, p.B, p.maxHW, s));
    if (d_hist && p.d_gt) KCHK(e, confusion_hist(d_labels, p.d_gt, desc, p.d_label_off, d_hist, n_class, p.B, p.maxHW, s));
    return PNP_OK;
}

extern "C" int pnp_postprocess(pnp_engine* e, const float* d_gradcam, int32_t T, float threshold, int32_t scale01, int32_t mode,
                               uint8_t* d_labels, unsigned long long* d_hist, int32_t n_class, void* stream) {
    if (int r = pnp_merge_tokens(e, d_gradcam, T, stream)) return r;
    if (int r = pnp_threshold_upsample(e, threshold, scale01, stream)) return r;
    if (mode & 1)
        if (int r = pnp_blur_minmax(e, stream)) return r;
    if (mode & 2)
        if (int r = pnp_densecrf(e, CRF_ITERS, CRF_POS_W, CRF_POS_XY, CRF_BI_W, CRF_BI_XY, CRF_BI_RGB, stream)) return r;
    return pnp_remap_hist(e, (mode & 2) ? 1 : 0, d_labels, d_hist, n_class, stream);
}

// 1-drop and N-drop "blur+crf" post-processing of one batch in ONE mean-field run (PnP.py:348-403 and 424-481 run the
// same DenseCRF twice per image on the same RGB image): the two problems become two channel groups of every row, so the
// lattice index walks -- contributor lists, neighbour ids, simplex offsets -- are shared.  Per-channel arithmetic is
// untouched: labels and histograms equal two pnp_postprocess calls bit for bit.
extern "C" int pnp_postprocess_pair(pnp_engine* e, const float* d_gradcam_1drop, const float* d_gradcam_ndrop, int32_t T,
                                    float threshold, int32_t scale01_mask, uint8_t* d_labels_1drop, unsigned long long* d_hist_1drop,
                                    uint8_t* d_labels_ndrop, unsigned long long* d_hist_ndrop, int32_t n_class, void* stream) {
    POST_READY(e);
    auto& p = e->post;
    if (!p.has_crf) return fail(e, PNP_ERR_STATE, "batch was prepared without CRF lattices");
    if (!d_labels_1drop || !d_labels_ndrop) return fail(e, PNP_ERR_ARG, "label outputs are null");
    if (p.groups_cap < 2) {                     // arrays sized for one group only: same results, two passes
        if (int r = pnp_postprocess(e, d_gradcam_1drop, T, threshold, scale01_mask & 1, 3, d_labels_1drop, d_hist_1drop, n_class, stream)) return r;
        return pnp_postprocess(e, d_gradcam_ndrop, T, threshold, (scale01_mask >> 1) & 1, 3, d_labels_ndrop, d_hist_ndrop, n_class, stream);
    }
    hipStream_t s = (hipStream_t)stream;
    for (int grp = 0; grp < 2; grp++) {
        if (int r = pnp_merge_tokens(e, grp == 0 ? d_gradcam_1drop : d_gradcam_ndrop, T, stream)) return r;
        // PnP.py: Scale_0_1 in the 1-drop branch only; PnPc.py: both
        if (int r = pnp_threshold_upsample(e, threshold, (scale01_mask >> grp) & 1, stream)) return r;
        if (int r = pnp_blur_minmax(e, stream)) return r;
        KCHK(e, unary_from_maps(p.maps2, p.view[1].d_desc, p.crf.unary, p.B, p.maxHW, p.maxKp, grp, s));
    }
    const CrfLabelOut lout{{d_labels_1drop, d_labels_ndrop}, p.d_lut, p.lut_stride, p.d_label_off};
    if (int r = crf_iterate(e, p.view[1], CRF_ITERS, CRF_POS_W, CRF_BI_W, s, lout)) return r;
    for (int grp = 0; grp < 2; grp++) {
        uint8_t* lab = grp == 0 ? d_labels_1drop : d_labels_ndrop;
        unsigned long long* hist = grp == 0 ? d_hist_1drop : d_hist_ndrop;
        if (hist && p.d_gt) KCHK(e, confusion_hist(lab, p.d_gt, p.view[0].d_desc, p.d_label_off, hist, n_class, p.B, p.maxHW, s));
    }
    return PNP_OK;
}

// ------------------------------------------------------------------------------------------ introspection

bool pnp::post_get_buffer(pnp_engine* e, const std::string& n, void** d_ptr, size_t* bytes) {
    auto& p = e->post;
    if (!p.reserved) return false;
    auto set = [&](void* ptr, size_t b) { *d_ptr = ptr; *bytes = b; return true; };
    const size_t mk = (size_t)p.max_total_pix * p.maxK * 4;
    const size_t mq = (size_t)p.max_total_pix * p.maxKp * 4 * p.groups_cap;   // as allocated: a paired run fills two groups per row
    if (n == "merged") return set(p.merged, (size_t)p.maxB * p.maxK * e->PP * 4);
    if (n == "maps") return set(p.maps_in_2 ? p.maps2 : p.maps, mk);
    if (n == "maps_pre_blur") return set(p.maps, mk);
    if (n == "unary") return set(p.crf.unary, mq);
    if (n == "crf_q") return set(p.crf.Q, mq);
    if (n == "crf_idbase_gauss") return set(p.crf.lat[0].idbase, ((size_t)p.maxB + 1) * 4);
    if (n == "crf_idbase_bilateral") return set(p.crf.lat[1].idbase, ((size_t)p.maxB + 1) * 4);
    if (n == "crf_norm_gauss") return set(p.crf.norm[0], (size_t)p.max_total_pix * 4);
    if (n == "crf_norm_bilateral") return set(p.crf.norm[1], (size_t)p.max_total_pix * 4);
    if (n == "crf_offset_gauss") return set(p.crf.lat[0].offset, (size_t)p.max_total_pix * 3 * 4);          // per pixel: 3 lattice ids
    if (n == "crf_offset_bilateral") return set(p.crf.lat[1].offset, (size_t)p.max_total_pix * 6 * 4);  // per pixel: 6 lattice ids
    if (n == "crf_nbr8_gauss") return set(p.crf.lat[0].nbr8, (size_t)(p.crf.lat[0].D1 / 2) * p.crf.lat[0].cap * sizeof(CrfNbr8));
    if (n == "crf_nbr8_bilateral") return set(p.crf.lat[1].nbr8, (size_t)(p.crf.lat[1].D1 / 2) * p.crf.lat[1].cap * sizeof(CrfNbr8));
    return false;
}
