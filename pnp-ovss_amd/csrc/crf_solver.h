// Internal to csrc/: the host side of the DenseCRF mean-field, shared by its two owners -- the engine's post-processing
// (pnp_engine::Post, post.hip) and the stand-alone solver (pnp_crf, crf_op.hip).  Host code only: the kernels and their
// launchers are in crf_lattice.hip, crf_meanfield.hip, crf_grad.hip and sort.hip (kernels.h).  Functions return PNP_* codes
// and format no text: each owner keeps its own error buffer, messages and allocator.
#pragma once
#include <vector>

#include "common.h"
#include "kernels.h"

namespace pnp {

constexpr int CRF_MAX_IMAGES = 64;                // IMG_BITS of the packed lattice key (crf_lattice.hip)
constexpr int CRF_MAX_LABELS = 255;               // uint8 labels
// |coordinate| a bilateral lattice key may reach: 11 bits per coordinate less the d + 1 = 6 of the canonical simplex
// (lattice_embed_kernel's range flag)
constexpr int CRF_KEY_LIMIT = (1 << 10) - 6;

// row stride of the pixel-major CRF arrays in floats: `groups` channel groups of K back to back, zero-padded to a multiple of 4
// (PostDesc::Kp; the paired run of K = 21 has rows of 44 instead of 2 x 24)
constexpr int crf_row_stride(int groups, int K) { return (groups * K + 3) / 4 * 4; }

struct CrfWorkspace {
    float *unary = nullptr, *Q = nullptr, *va = nullptr, *vb = nullptr, *vga = nullptr, *vgb = nullptr, *norm[2] = {nullptr, nullptr};
    CrfLattice lat[2]{};                          // [0] Gaussian, [1] bilateral
    CrfBuildScratch scratch{};
    size_t val_cap = 0, valg_cap = 0;             // floats of the bilateral (va, vb) / Gaussian (vga, vgb) lattice value buffers
    std::vector<double> gauss_sig;                // what the Gaussian lattice was last built for: its widths (sx, sy), then H, W of every image
    int lat_points[2] = {0, 0};                   // lattice points of the last build (Gaussian, bilateral)
    // Feature terms (crf_reserve_plan with max_terms > 0): one lattice of up to max_dims axes and one normaliser per term, each
    // sized for the worst case of max_dims + 1 lattice points per pixel.  The terms take turns in va / vb -- a term's filtered
    // values are consumed by its own update launch -- and add into the pixel-major rows of `logit`
    int max_terms = 0, max_dims = 0;
    std::vector<CrfLattice> tlat;
    std::vector<float*> tnorm;
    std::vector<int> tlat_points;
    float* logit = nullptr;
};

// One device allocation of the workspace: the owner allocates `bytes` with its own allocator (its list, its byte count),
// zero-filled if `zero`, and stores the pointer in *dst
struct CrfAlloc {
    void** dst;
    size_t bytes;
    bool zero;
};
// The workspace's allocations, in order, for batches of at most `images` images and `total_pix` pixels, rows of `groups` channel
// groups of at most max_kp floats each, and lattice value buffers for the rows of `value_pix` pixels at once (a chunk of the
// batch; total_pix: all of it).  max_terms > 0: also up to that many feature-term lattices of 1 .. max_dims axes (build scratch
// for max_dims + 1 entries per pixel, value buffers for max_dims + 1 rows per pixel).  Sets the capacities of `ws`.
std::vector<CrfAlloc> crf_reserve_plan(CrfWorkspace& ws, size_t images, size_t total_pix, size_t value_pix, size_t max_kp, size_t groups,
                                       size_t max_terms = 0, size_t max_dims = 0);

struct CrfOffsets {                               // running offsets of a batch layout
    int64_t pix = 0;
    size_t off = 0, qoff = 0, voff[2] = {0, 0};
};
// Where d (H, W, K are set) lies in a batch with `groups` channel groups per row -- pix0, off, G, Kp, qoff, voff -- and `at`
// advanced past it.  False: beyond the per-image addressing of the iteration kernels (24-bit row ids, 32-bit byte offsets: crf_meanfield.hip)
bool crf_layout_image(PostDesc& d, int groups, CrfOffsets& at);

// Both lattices of a batch (the features are fixed per batch) and their normalisers.  The Gaussian (xy-only) lattice depends on
// the image sizes and pos_xy alone and is kept across batches; every lattice built synchronises once (size + range flag
// read-back).  A raised key-range flag ends the build at that lattice: PNP_ERR_ARG with *range_term = 0 (Gaussian) / 1
// (bilateral), else -1; the device flag is cleared and no lattice is kept, so the next build makes both.
int crf_build(CrfWorkspace& ws, const PostDesc* d_desc, const PostDesc* h_desc, int B, size_t total_pix, int maxHW, const uint8_t* d_rgb,
              const float pos_xy[2], const float bi_xy[2], const float bi_rgb[3], int* range_term, hipStream_t s);

// The lattices and normalisers of T feature terms (ws.tlat / ws.tnorm [0, T)): term t has dims[t] = 1 .. ws.max_dims feature planes
// per image in d_feat[t] (crf_build_lattice_features).  One synchronisation per lattice.  A raised range flag (a coordinate
// beyond the key, a non-finite feature) ends the build: PNP_ERR_ARG with *range_term = that term, else -1; the flag is cleared.
int crf_build_terms(CrfWorkspace& ws, const PostDesc* d_desc, const PostDesc* h_desc, int B, size_t total_pix, int maxHW, int T,
                    const int* dims, const float* const* d_feat, int* range_term, hipStream_t s);

// What a T-term update takes besides the workspace: per term its descriptors (device; PostDesc::voff[0] = the term's value
// rows), and its compatibility -- MT[t] (K x K message weights, transposed as crf_update_compat takes them) or else wvec[t] (one
// weight per label, ldm floats) or else the scalar w[t]
struct CrfTermsRun {
    int T;
    const PostDesc* const* d_desc;
    const float* w;
    const float* const* wvec;
    const float* const* MT;
    int ldm;
};

struct CrfSpan {                                  // the images [img0, img0 + nimg) of one layout of a batch
    const PostDesc* d_desc;
    int img0, nimg;
    int kp_max;                                   // widest row of the batch, floats
    int groups;
};
// one filter pass per term at the current Q, which stays as it is: *rg / *rb = the filtered values
int crf_meanfield_filter(const CrfWorkspace& ws, const CrfSpan& v, const float** rg, const float** rb, hipStream_t s);
// The mean-field on the images of v, in the order start, updates.  labels: the label output, asked of the launch that leaves
// the final marginals -- of the start when no update follows, else of the last update.
// Q0 = softmax(-U)
int crf_meanfield_start(const CrfWorkspace& ws, const CrfSpan& v, hipStream_t s, const CrfLabelOut& labels);
// What a two-term update takes: the weights of the Potts kernel or, MgT non-null, the matrices of the compatibility kernel
// (MgT, MbT, ldm as crf_update_compat takes them; one group only)
struct CrfPairRun {
    float pos_w, bi_w;
    const float *MgT, *MbT;
    int ldm;
};
// n updates from the current Q, each both filters and the update kernel
int crf_meanfield(const CrfWorkspace& ws, const CrfSpan& v, int n, const CrfPairRun& run, hipStream_t s, const CrfLabelOut& labels);
// n updates from the current Q, each the T feature terms in order -- filter, then crf_term_update into the logit rows, the last
// one ending in the softmax
int crf_meanfield_terms(const CrfWorkspace& ws, const CrfSpan& v, int n, const CrfTermsRun& terms, hipStream_t s, const CrfLabelOut& labels);

// The gradient workspace of a solver of feature terms (pnp_crf_reserve_grad): rows as Q -- g (the cotangent of the marginals,
// rewritten in place update by update), dl, h, gU (the unary gradient) --, the per-tile partials of one term's compatibility
// gradient (part_cap >= max_psz floats), their per-image fp64 sums (images x max_psz) and the running sums acc[term][max_psz], and the
// first tile of every image (tile0: images + 1)
struct CrfGradWorkspace {
    float *g = nullptr, *dl = nullptr, *h = nullptr, *gU = nullptr, *part = nullptr;
    double *img_sum = nullptr, *acc = nullptr;
    int* tile0 = nullptr;
    size_t part_cap = 0, max_psz = 0;
};
// Reverse mode over n updates of the T feature terms of `terms` on the images of v (crf_meanfield_terms).  history: the
// n + 1 iterates Q_0 .. Q_n, q_floats apart, as ws.Q held them; gw.g: the cotangent of Q_n on entry.  On return gw.gU holds the
// gradient of the unary rows and, for every term with psz[t] > 0 (1, K or K * K: the floats of its compatibility), gw.acc +
// t * gw.max_psz the fp64 gradient of its compatibility; only those terms pay a forward filter per update.  h_tile0: tile0 on
// the host (crf_backward_tiles per image).  Reads ws.unary's layout only; uses ws.va / ws.vb; ws.Q is not touched.  A term's
// partials go through gw.part (>= max_psz floats) in spans -- whole images while they fit, else the tiles of one image in runs --
// and the fp64 sums carry over the spans, so the result does not depend on part_cap
int crf_meanfield_backward(const CrfWorkspace& ws, const CrfGradWorkspace& gw, const CrfSpan& v, int max_pixels, int n, const CrfTermsRun& terms,
                           const float* history, size_t q_floats, const int* psz, const int* h_tile0, hipStream_t s);

}  // namespace pnp
