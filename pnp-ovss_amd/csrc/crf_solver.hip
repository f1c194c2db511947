// The DenseCRF host side of crf_solver.h.  Host logic only: every kernel is behind a launcher of kernels.h.
#include "crf_solver.h"

#include <algorithm>
#include <climits>

namespace pnp {

std::vector<CrfAlloc> crf_reserve_plan(CrfWorkspace& ws, size_t B, size_t TP, size_t value_pix, size_t Kp, size_t groups, size_t max_terms,
                                       size_t max_dims) {
    std::vector<CrfAlloc> plan;
    auto want = [&plan](size_t count, bool zero, auto**... dst) {      // `count` elements for each of dst, in order
        (plan.push_back({reinterpret_cast<void**>(dst), count * sizeof(**dst), zero}), ...);
    };
    auto want_lattice = [&](CrfLattice& L, size_t D1, int which) {     // a lattice's arrays for D1 points per pixel at most
        L.D1 = (int)D1;
        L.which = which;
        L.cap = TP * D1;
        want(L.cap, false, &L.bary, &L.vals, &L.ent, &L.offset);
        want(L.cap + 1, false, &L.seg_start);
        want(L.cap, false, &L.seg_lo, &L.seg_hi, &L.ukeys);
        want(B + 1, false, &L.idbase);
        want(L.cap * D1, false, &L.n1, &L.n2);
        want(L.cap * (D1 / 2), false, &L.nbr8);
    };
    want(TP * Kp * groups, false, &ws.unary, &ws.Q);
    want(TP, false, &ws.norm[0], &ws.norm[1]);
    want_lattice(ws.lat[0], 3, 0);
    want_lattice(ws.lat[1], 6, 1);
    // feature terms: every lattice for the worst case of max_dims + 1 points per pixel
    const size_t tD1 = max_terms ? max_dims + 1 : 0;
    ws.max_terms = (int)max_terms;
    ws.max_dims = (int)max_dims;
    ws.tlat.assign(max_terms, CrfLattice{});
    ws.tnorm.assign(max_terms, nullptr);
    ws.tlat_points.assign(max_terms, 0);
    for (size_t t = 0; t < max_terms; t++) {
        want_lattice(ws.tlat[t], tD1, 1);         // (crf_build_terms sets the term's own d + 1)
        want(TP, false, &ws.tnorm[t]);
    }
    if (max_terms) want(TP * Kp * groups, false, &ws.logit);
    const size_t rows = std::max<size_t>(6, tD1);  // lattice points per pixel at most, over every lattice of the workspace
    const size_t cap6 = TP * rows;                // E of CrfBuildScratch (kernels.h)
    CrfBuildScratch& sc = ws.scratch;
    want(cap6, false, &sc.keys_a, &sc.keys_b, &sc.vals_a, &sc.head, &sc.incl);
    want(cap6 * rows, false, &sc.n1k, &sc.n2k);
    want(1, true, &sc.range_err);
    sc.temp_bytes = crf_sort_temp_bytes(cap6);
    want(sc.temp_bytes, false, &sc.temp);
    // lattice value buffers: one row per lattice point, at most 6 (bilateral) / 3 (Gaussian) points per pixel;
    // crf_lattice_norm also uses va / vb as scalar scratch of one float per lattice point of the whole batch
    ws.val_cap = std::max(value_pix * rows * Kp * groups, cap6);
    want(ws.val_cap, false, &ws.va, &ws.vb);
    ws.valg_cap = value_pix * 3 * Kp * groups;
    want(ws.valg_cap, false, &ws.vga, &ws.vgb);
    return plan;
}

bool crf_layout_image(PostDesc& d, int groups, CrfOffsets& at) {
    const int64_t n = (int64_t)d.H * d.W;
    d.pix0 = (int)at.pix;
    d.off = at.off;
    at.pix += n;
    at.off += (size_t)n * d.K;
    d.G = groups;
    d.Kp = crf_row_stride(groups, d.K);
    d.qoff = at.qoff;
    at.qoff += (size_t)n * d.Kp;
    for (int t = 0; t < 2; t++) {
        d.voff[t] = at.voff[t];
        at.voff[t] += (size_t)n * (t == 0 ? 3 : 6) * d.Kp;
    }
    return n * 6 < (1 << 24) && n * 6 * d.Kp * 4 < ((int64_t)1 << 32);
}

// One lattice of a batch and its normaliser: over the feature planes d_feat or, null, over the pixel positions and d_rgb with
// the widths sxy, srgb.  A raised key-range flag is cleared on the device: *raised, PNP_ERR_ARG
static int crf_build_one(CrfWorkspace& ws, CrfLattice& L, float* norm, int* points, const PostDesc* d_desc, const PostDesc* h_desc, int B,
                         size_t total_pix, int maxHW, const uint8_t* d_rgb, const float* sxy, const float* srgb, const float* d_feat,
                         bool* raised, hipStream_t s) {
    const size_t entries = total_pix * L.D1;
    int range_err = 0;
    if (int r = d_feat ? crf_build_lattice_features(L.D1 - 1, L, d_desc, h_desc, d_feat, B, entries, maxHW, ws.scratch, &range_err, points, s)
                       : crf_build_lattice(L.D1 - 1, L, d_desc, h_desc, d_rgb, sxy, srgb, B, entries, maxHW, ws.scratch, &range_err, points, s))
        return r;
    if (int r = crf_lattice_norm(L, d_desc, B, maxHW, entries, ws.va, ws.vb, norm, s)) return r;
    *raised = range_err != 0;
    if (!range_err) return PNP_OK;
    (void)hipMemsetAsync(ws.scratch.range_err, 0, sizeof(int), s);
    return PNP_ERR_ARG;
}

int crf_build(CrfWorkspace& ws, const PostDesc* d_desc, const PostDesc* h_desc, int B, size_t total_pix, int maxHW, const uint8_t* d_rgb,
              const float pos_xy[2], const float bi_xy[2], const float bi_rgb[3], int* range_term, hipStream_t s) {
    std::vector<double> sig = {pos_xy[0], pos_xy[1]};
    for (int i = 0; i < B; i++) { sig.push_back(h_desc[i].H); sig.push_back(h_desc[i].W); }
    *range_term = -1;
    for (int t = 0; t < 2; t++) {
        if (t == 0 && sig == ws.gauss_sig) continue;
        if (t == 0) ws.gauss_sig.clear();         // until the new one stands
        bool raised = false;
        if (int r = crf_build_one(ws, ws.lat[t], ws.norm[t], &ws.lat_points[t], d_desc, h_desc, B, total_pix, maxHW, d_rgb,
                                  t == 0 ? pos_xy : bi_xy, bi_rgb, nullptr, &raised, s)) {
            if (raised) {                         // leave no stale state behind
                ws.gauss_sig.clear();
                *range_term = t;
            }
            return r;
        }
        if (t == 0) ws.gauss_sig = sig;
    }
    return PNP_OK;
}

int crf_build_terms(CrfWorkspace& ws, const PostDesc* d_desc, const PostDesc* h_desc, int B, size_t total_pix, int maxHW, int T,
                    const int* dims, const float* const* d_feat, int* range_term, hipStream_t s) {
    *range_term = -1;
    if (T < 1 || T > ws.max_terms) return PNP_ERR_ARG;
    for (int t = 0; t < T; t++) {
        if (dims[t] < 1 || dims[t] > ws.max_dims) return PNP_ERR_ARG;
        ws.tlat[t].D1 = dims[t] + 1;
        bool raised = false;
        if (int r = crf_build_one(ws, ws.tlat[t], ws.tnorm[t], &ws.tlat_points[t], d_desc, h_desc, B, total_pix, maxHW, nullptr, nullptr, nullptr,
                                  d_feat[t], &raised, s)) {
            if (raised) *range_term = t;
            return r;
        }
    }
    return PNP_OK;
}

int crf_meanfield_filter(const CrfWorkspace& ws, const CrfSpan& v, const float** rg, const float** rb, hipStream_t s) {
    if (int r = crf_filter(ws.lat[0], v.d_desc, v.img0, v.nimg, ws.Q, ws.vga, ws.vgb, rg, v.kp_max, s)) return r;
    return crf_filter(ws.lat[1], v.d_desc, v.img0, v.nimg, ws.Q, ws.va, ws.vb, rb, v.kp_max, s);
}

int crf_meanfield_start(const CrfWorkspace& ws, const CrfSpan& v, hipStream_t s, const CrfLabelOut& labels) {
    return crf_update(ws.lat[0], ws.lat[1], v.d_desc, v.img0, v.nimg, ws.vga, ws.va, ws.norm[0], ws.norm[1], ws.unary, ws.Q, 0.f, 0.f, 0,
                      v.kp_max, v.groups, s, labels);
}

int crf_meanfield(const CrfWorkspace& ws, const CrfSpan& v, int n, const CrfPairRun& run, hipStream_t s, const CrfLabelOut& labels) {
    for (int it = 0; it < n; it++) {
        const float *rg = nullptr, *rb = nullptr;
        if (int r = crf_meanfield_filter(ws, v, &rg, &rb, s)) return r;
        const CrfLabelOut out = it == n - 1 ? labels : CrfLabelOut();
        const int r = run.MgT ? crf_update_compat(ws.lat[0], ws.lat[1], v.d_desc, v.img0, v.nimg, rg, rb, ws.norm[0], ws.norm[1], ws.unary, ws.Q,
                                                  run.MgT, run.MbT, run.ldm, v.kp_max, s, out, nullptr)
                              : crf_update(ws.lat[0], ws.lat[1], v.d_desc, v.img0, v.nimg, rg, rb, ws.norm[0], ws.norm[1], ws.unary, ws.Q,
                                           run.pos_w, run.bi_w, 1, v.kp_max, v.groups, s, out);
        if (r) return r;
    }
    return PNP_OK;
}

int crf_meanfield_terms(const CrfWorkspace& ws, const CrfSpan& v, int n, const CrfTermsRun& terms, hipStream_t s, const CrfLabelOut& labels) {
    for (int it = 0; it < n; it++)
        for (int t = 0; t < terms.T; t++) {
            const bool first = t == 0, last = t == terms.T - 1;
            const float* val = nullptr;
            if (int r = crf_filter(ws.tlat[t], terms.d_desc[t], v.img0, v.nimg, ws.Q, ws.va, ws.vb, &val, v.kp_max, s)) return r;
            if (int r = crf_term_update(ws.tlat[t], terms.d_desc[t], v.img0, v.nimg, val, ws.tnorm[t], first ? ws.unary : ws.logit, first,
                                        last ? ws.Q : ws.logit, last, terms.w[t], terms.wvec[t], terms.MT[t], terms.ldm, v.kp_max, s,
                                        last && it == n - 1 ? labels : CrfLabelOut()))
                return r;
        }
    return PNP_OK;
}

int crf_meanfield_backward(const CrfWorkspace& ws, const CrfGradWorkspace& gw, const CrfSpan& v, int max_pixels, int n, const CrfTermsRun& terms,
                           const float* history, size_t q_floats, const int* psz, const int* h_tile0, hipStream_t s) {
    if (hipMemsetAsync(gw.gU, 0, q_floats * sizeof(float), s) != hipSuccess) return PNP_ERR_HIP;
    for (int t = 0; t < terms.T; t++)
        if (psz[t] > 0 && hipMemsetAsync(gw.acc + (size_t)t * gw.max_psz, 0, (size_t)psz[t] * sizeof(double), s) != hipSuccess) return PNP_ERR_HIP;
    for (int it = n; it >= 1; it--) {
        const float* const Qi = history + (size_t)it * q_floats;
        const float* const Qprev = history + (size_t)(it - 1) * q_floats;
        if (int r = crf_softmax_backward(v.d_desc, v.img0, v.nimg, Qi, gw.g, gw.dl, gw.gU, max_pixels, v.kp_max, s)) return r;
        for (int t = 0; t < terms.T; t++) {                  // (gw.g is free from here on: the terms' slices rebuild it)
            const CrfLattice& L = ws.tlat[t];
            if (psz[t] > 0) {
                // the message of the update is recomputed, and the images go in spans whose partials the buffer holds
                const float* val = nullptr;
                if (int r = crf_filter(L, terms.d_desc[t], v.img0, v.nimg, Qprev, ws.va, ws.vb, &val, v.kp_max, s)) return r;
                const int cap_tiles = (int)std::min<size_t>(gw.part_cap / psz[t], INT_MAX);      // >= 1: part_cap >= max_psz
                double* const acc = gw.acc + (size_t)t * gw.max_psz;
                for (int i0 = v.img0; i0 < v.img0 + v.nimg;) {
                    int ni = 0;
                    while (i0 + ni < v.img0 + v.nimg && h_tile0[i0 + ni + 1] - h_tile0[i0] <= cap_tiles) ni++;
                    // whole images while they fit; an image with more tiles than the buffer holds goes in spans of its tiles
                    const int ntiles = ni ? INT_MAX : h_tile0[i0 + 1] - h_tile0[i0];
                    for (int t_lo = 0; t_lo < ntiles; t_lo += cap_tiles) {
                        const int t_hi = ni ? INT_MAX : std::min(t_lo + cap_tiles, ntiles);
                        if (int r = crf_term_backward(L, terms.d_desc[t], i0, ni ? ni : 1, val, ws.tnorm[t], gw.dl, gw.h, terms.w[t],
                                                      terms.wvec[t], terms.MT[t], terms.ldm, v.kp_max, gw.part, gw.tile0, psz[t], t_lo, t_hi, s))
                            return r;
                        if (int r = crf_grad_reduce(gw.part, gw.tile0, i0, ni ? ni : 1, psz[t], gw.img_sum, acc, t_lo, t_hi, t_hi >= ntiles, s))
                            return r;
                        if (ni) break;
                    }
                    i0 += ni ? ni : 1;
                }
            } else if (int r = crf_term_backward(L, terms.d_desc[t], v.img0, v.nimg, nullptr, ws.tnorm[t], gw.dl, gw.h, terms.w[t],
                                                 terms.wvec[t], terms.MT[t], terms.ldm, v.kp_max, nullptr, nullptr, 0, 0, INT_MAX, s)) {
                return r;
            }
            const float* valT = nullptr;
            if (int r = crf_filter(L, terms.d_desc[t], v.img0, v.nimg, gw.h, ws.va, ws.vb, &valT, v.kp_max, s, true)) return r;
            if (int r = crf_slice_add(L, terms.d_desc[t], v.img0, v.nimg, valT, ws.tnorm[t], gw.g, t == 0, s)) return r;
        }
    }
    // Q_0 = softmax(-U)
    return crf_softmax_backward(v.d_desc, v.img0, v.nimg, history, gw.g, gw.dl, gw.gU, max_pixels, v.kp_max, s);
}

}  // namespace pnp
