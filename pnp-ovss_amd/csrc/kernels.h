// Host launchers of the hand-written gfx950 kernels (one .hip per group).  All return PNP_OK or a
// negative errno-style code; none allocates or synchronises (graph-capture safe).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "gemm.h"

namespace pnp {

// Per-image descriptor of the post-process batch (images may have different original sizes and
// class counts).  `off` = offset (in floats) of this image's K*H*W block inside the flat map /
// unary / Q / tmp buffers; `pix0` = global index of its first pixel; `voff[t]` = offset of its
// lattice value block (t = 0 Gaussian, 1 bilateral; the descriptors of a feature term carry that term's offset in both).
struct PostDesc {
    int H, W, K, C, has_bg, pix0;
    int Kp;            // row stride of the CRF arrays in floats: G groups of Kg back to back, zero-padded to a multiple of 4
    int G, Kg;         // channel groups per row (1; 2 = the 1-drop and N-drop problems of one batch side by side, which
                       // share every lattice index walk) and floats per group (= K)
    size_t off;        // K*H*W blocks of the (K,H,W) map buffers
    size_t qoff;       // Kp*H*W blocks of the pixel-major CRF arrays (unary, Q)
    size_t voff[2];
};

// contributor record of a lattice point, stored in list order: global pixel index, barycentric weight, the pixel's
// normaliser 1/sqrt(lattice(1) + 1e-20) (filled in by crf_lattice_norm); one 16-byte load per contributor
struct alignas(16) CrfEntry {
    uint32_t pixel;
    float w;
    float nr;
    uint32_t pad;
};

// neighbour record of the two-axis lattice blur (crf_blur4x2_kernel): image-local lattice ids, -1 = absent
struct alignas(16) CrfNbr8 {
    int ia, id;        // neighbours along the pair's first axis
    int pa, pd;        // neighbours along its second axis ...
    int aa, ad;        // ... and their neighbours along the first axis
    int da, dd;
};

// One permutohedral lattice type for a whole image batch (device pointers).
struct CrfLattice {
    int D1;            // d + 1
    int which;         // 0 Gaussian, 1 bilateral: the PostDesc::voff its value rows use (a feature term: 1, both voff equal)
    size_t cap;        // capacity (entries) = stride of the neighbour tables
    float* bary;       // [entries] barycentric weight per (pixel, vertex)
    uint32_t* vals;    // [entries] sorted (pixel, vertex) indices = contributor lists
    CrfEntry* ent;     // [entries] the same lists as (pixel, weight, norm) records (what the splat streams)
    int* offset;       // [entries] lattice id per (pixel, vertex)
    int* seg_start;    // [M+1] first sorted entry of each lattice point, key order (build scratch)
    int* seg_lo;       // [M] contributor range of each lattice point (final, spatial numbering)
    int* seg_hi;
    uint64_t* ukeys;   // [M] sorted unique packed keys
    int* idbase;       // [B+1] first lattice id of each image
    int* n1;           // [(d+1) * cap]
    int* n2;
    CrfNbr8* nbr8;     // [(d+1)/2 * cap] per axis pair
};

// vit_kernels.hip
int patchify(int bf, const float* img, const uint8_t* dropped, void* out, int B, int S, int P, hipStream_t s);
int cls_rows(const float* cls, const float* pos, float* x, int B, int N, int D, hipStream_t s);
int layernorm(int bf, const float* x, const float* w, const float* b, float eps, int rows, int D, float* y, void* yt,
              float* xhat, float* rstd, hipStream_t s, void* yt_lo = nullptr);
int vit_attention(int bf, const void* qk, int ld_qk, int D, const void* vt, int ld_vt, int Npad, void* ctx, int B,
                  int H, int N, float scale, hipStream_t s, void* ctx_lo = nullptr);

int vit_attention_x3(const void* qkv_hi, const void* qkv_lo, int ld_qk, int D, void* ctx_hi, void* ctx_lo, int B, int H, int N,
                     float scale, hipStream_t s);

// text_kernels.hip
// enc_id >= 0: column 0 of every row is replaced by that id ([ENC], the multimodal pass); enc_id < 0: column 0 kept as given
int text_embed(const int64_t* ids, int ld_ids, const float* word, const float* pos, float* out, int B, int L, int H,
               int enc_id, int vocab, hipStream_t s);
// scratch: [B, heads, L, L] floats, used when L > 192 and probs is null (the long-caption form passes a row's probabilities
// through global memory)
int text_self_attn(int bf, const void* qkv, const int64_t* mask, int ld_mask, void* ctx, float* probs, float* scratch, int B, int L,
                   int H, hipStream_t s);
void set_text_rows(int n);   // 0 = cost model, 1..4 = workgroups per (head, image) of the row-split self-attention launches
int text_self_attn_bwd(int bf, const void* qkv, const float* dctx, const float* probs, float* ds_scratch, void* dqkv,
                       int B, int L, int H, hipStream_t s);
int xattn(int bf, int mode, const void* a1, int ld1, const void* a2t, int ld2, int Npad, const void* x, int ldx,
          void* out, int ldo, float* pbuf, int Nst, int B, int L, int N, int nheads, hipStream_t s);
int layernorm_bwd(int bf, const float* dy, const float* w, const float* xhat, const float* rstd, int rows, int D,
                  float* dx, void* dxt, hipStream_t s);
int itm_head(const float* hlast, const float* w, const float* bias, float* logits, int B, int L, int H, hipStream_t s);
int itm_grad_seed(const float* w, float* dh, int B, int L, int H, hipStream_t s);
int cast_f32(int bf, const float* in, void* out, size_t n, hipStream_t s);
int split_f32(const float* in, void* hi, void* lo, size_t n, hipStream_t s);     // x ~ hi + lo, both bf16 (round to nearest even)

// itc_kernels.hip
int l2_normalize_rows(float* x, int rows, int E, float eps, hipStream_t s);                  // in place: x / max(||x||_2, eps)
int itc_similarity(const float* img, const float* txt, float* sim, int B, int T, int E, hipStream_t s);   // sim = img . txt^T, fp32 FMA
int cast_rows_bf16(const float* in, int ld_in, void* out, int rows, int K, hipStream_t s);   // strided fp32 rows -> contiguous bf16

// pipeline_kernels.hip
int gradcam_gather(const float* P, const float* dP, const int64_t* mask, int ld_mask, float* out, int B, int nheads,
                   int head, int L, int Nst, int PP, hipStream_t s);
int drop_step(const float* G, float* g0, float* agg, uint8_t* dropped, int32_t* picks, int iter, int B, int T, int PP,
              int npick, int max_picks, hipStream_t s);
int merge_tokens(const float* src, const int32_t* cls_off, const int32_t* tok_idx, const int32_t* cls_div,
                 const int32_t* img_cls_off, float* out, int B, int T, int PP, int Cmax, hipStream_t s);
int threshold_maps(const float* merged, const int32_t* img_cls_off, float* out, float threshold, int B, int PP, int Cmax,
                   hipStream_t s);
int upsample_maps(const float* src, const PostDesc* desc, float* maps, int B, int P, int Cmax, int maxHW, hipStream_t s);
int minmax_normalize(float* maps, const PostDesc* desc, float* stats, int B, int Kmax, int maxHW, int class_channels_only,
                     hipStream_t s);
int background_channel(float* maps, const PostDesc* desc, int B, int maxHW, hipStream_t s);
int blur_maps(const float* in, float* tmp, float* out, const PostDesc* desc, const double* wts, const int32_t* wt_off,
              int B, int Kmax, int maxH, int maxW, int max_radius, hipStream_t s);
int preprocess_images(const uint8_t* rgb, const void* desc, int B, int S, int max_H, const int32_t* coef, uint8_t* tmp,
                      const float* mean3, const float* std3, float* out, hipStream_t s);
int unary_from_maps(const float* maps, const PostDesc* desc, float* unary, int B, int maxHW, int max_kp, int group, hipStream_t s);
int argmax_remap(const float* q, const PostDesc* desc, const int32_t* lut, int lut_stride, uint8_t* labels,
                 const size_t* label_off, int pixel_major, int group, int B, int maxHW, hipStream_t s);
int confusion_hist(const uint8_t* labels, const float* gt, const PostDesc* desc, const size_t* label_off,
                   unsigned long long* hist, int n_class, int B, int maxHW, hipStream_t s);

// jpeg.hip -- descriptors shared with the host (pnp_ovss/jpeg.py mirrors them with ctypes; see include/pnp_hip.h)
struct JpegImage {
    int64_t data_off;       // offset of the entropy-coded segment in d_data (16-byte aligned)
    int64_t coef_off[3];    // int16 elements: component coefficient blocks [blocks_y][blocks_x][64], natural order
    int64_t plane_off[3];   // bytes: component sample planes, row stride blocks_x * 8
    int64_t rgb_off;        // bytes: output RGB, H * W * 3
    int32_t data_len, H, W, ncomp, hmax, vmax, mcux, mcuy;
    int32_t h[3], v[3], tq[3], td[3], ta[3], bx[3], by[3];
    int32_t tab, pad[2];
};
struct JpegTables {
    uint8_t counts[4][16];  // [DC0, DC1, AC0, AC1]: the file's DHT segments as they are (codes per length 1..16, symbols)
    uint8_t vals[4][256];
    int32_t quant[4][64];   // natural (row-major) order
};
struct JpegSegment {
    int64_t byte_off;       // first entropy-coded byte of the restart interval, relative to the image's data_off
    int64_t clean_off;      // where its un-stuffed bytes go in d_clean (16-byte aligned)
    int32_t image, mcu0, nmcu;
    int32_t raw_len;        // entropy-coded bytes of the interval (markers excluded)
    int32_t clean_cap;      // bytes reserved at clean_off: >= raw_len + 32
    int32_t sub_bits;       // sub-sequence length of the parallel decode: a multiple of 32, >= 8 * raw_len / 1024
    int32_t scan;           // jpeg_decode_scans: index of the segment's JpegScan; mcu0 / nmcu then count that scan's units
    int32_t pad;
};
int jpeg_decode(const uint8_t* d_data, const JpegImage* d_imgs, const JpegTables* d_tabs, const JpegSegment* d_segs, int n_images,
                int n_segments, uint8_t* d_clean, int* d_seg_bits, int16_t* d_coef, size_t coef_elems, uint8_t* d_planes, uint8_t* d_rgb,
                int max_blocks, int max_pixels, int* d_err, hipStream_t s);
// the launches of jpeg_decode one stage at a time (un-stuff; baseline entropy decode; inverse DCT + colour)
void jpeg_launch_unstuff(const uint8_t* d_data, const JpegImage* d_imgs, const JpegSegment* d_segs, int n_segments, uint8_t* d_clean,
                         int* d_seg_bits, hipStream_t s);
void jpeg_launch_huffman(const uint8_t* d_clean, const JpegImage* d_imgs, const JpegTables* d_tabs, const JpegSegment* d_segs,
                         int n_segments, const int* d_seg_bits, int16_t* d_coef, int* d_err, hipStream_t s);
void jpeg_launch_pixels(const JpegImage* d_imgs, const JpegTables* d_tabs, int n_images, const int16_t* d_coef, uint8_t* d_planes,
                        uint8_t* d_rgb, int max_blocks, int max_pixels, hipStream_t s);

// jpeg_prog.hip -- progressive files scan by scan (pnp_ovss/jpeg.py pack_scans; see include/pnp_hip.h)
struct JpegScan {
    int32_t image;
    int32_t kind;           // 0 sequential (a baseline file's one scan), 1 DC first, 2 DC refinement, 3 AC first, 4 AC refinement
    int32_t ordinal;        // position of the scan in its file
    int32_t ncomp, comp[3]; // the scan's components: indices into the frame
    int32_t td[3], ta[3];   // per scan component: slot (0 / 1) of its DC / AC table in JpegTables `tab`
    int32_t ss, se, ah, al;
    int32_t tab;            // the Huffman tables in force at this SOS
    int32_t bw, bh;         // grid of the scan's units: MCUs when interleaved, the component's own blocks for one component
    int32_t nunits;
    int32_t pad[3];
};
int jpeg_decode_scans(const uint8_t* d_data, const JpegImage* d_imgs, const JpegTables* d_tabs, const JpegScan* d_scans,
                      const JpegSegment* d_segs, int n_images, int n_segments, int n_base_segments, const int32_t* h_groups, int n_groups,
                      uint8_t* d_clean, int* d_seg_bits, int16_t* d_coef, size_t coef_elems, uint64_t* d_hist, uint8_t* d_planes,
                      uint8_t* d_rgb, int max_blocks, int max_pixels, int* d_rounds, float* h_group_ms, int* d_err, hipStream_t s);

// sort.hip: stable LSD radix sort of (u64 key, u32 value) pairs and int32 prefix sum (the lattice build's device-wide primitives)
size_t sort_temp_bytes(size_t n);
int radix_sort_pairs(uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n, int begin_bit, int end_bit,
                     const size_t* seg_off, int nseg, void* temp, size_t temp_bytes, hipStream_t s);
int device_scan_i32(const int* in, int* out, size_t n, bool inclusive, void* temp, size_t temp_bytes, hipStream_t s);
// crf_lattice.hip: the lattice build and the normaliser
size_t crf_sort_temp_bytes(size_t max_entries);
// Device scratch of crf_build_lattice, sized once for the largest build: E = (pixels of a batch) x 6 entries of the bilateral
// lattice (the Gaussian one has 3 per pixel; a workspace with feature terms: x max(6, max_dims + 1), and n1k / n2k that many rows
// of stride E), M <= E lattice points.  The build reuses the arrays as it goes:
//   keys_a  [E] u64   packed (pixel, vertex) keys, the first sort's input; then the second sort's input keys [M];
//                     then, as int [M], the contributor-list lengths
//   keys_b  [E] u64   the first sort's output; then the second sort's output keys [M]; then, as u32 [E], the moved contributor list
//   vals_a  [E] u32   entry indices, the first sort's input; then the second sort's input ids [M]
//   head    [E] int   segment-head flags; then the spatial rank of every lattice point [M]
//   incl    [E] int   inclusive scan of `head`; then, as u32 [M], the second sort's output ids; then the new list starts [M]
//   n1k/n2k [6 E] int neighbour ids in key order, (d + 1) rows of stride CrfLattice::cap
//   temp              sort / scan workspace of temp_bytes >= crf_sort_temp_bytes(E)
//   range_err   int   device flag, zero on entry: set when a coordinate does not fit the packed key
struct CrfBuildScratch {
    uint64_t *keys_a, *keys_b;
    uint32_t* vals_a;
    int *head, *incl, *n1k, *n2k;
    char* temp;
    size_t temp_bytes;
    int* range_err;
};
// h_range_err: set to 1 when the flag was raised (read back with the lattice size: the build's one synchronisation)
int crf_build_lattice(int D, const CrfLattice& L, const PostDesc* d_imgs, const PostDesc* h_imgs, const uint8_t* d_rgb, const float sxy[2],
                      const float srgb[3], int B, size_t ent_total, int max_pixels, const CrfBuildScratch& scratch, int* h_range_err, int* h_points,
                      hipStream_t s);
// The same build on D = 1 .. 6 feature planes the caller brings (pnp_crf_set_batch_terms): d_feat holds image b's (D, H*W) block
// at float offset pix0 * D, the features already divided by their widths.  The flag is raised for a coordinate beyond
// crf_feature_key_limit(D) -- what the key's min(16, 64 / D) bits per coordinate hold, 505 at D = 6 -- and for a non-finite
// feature.  Scratch for E = (pixels of the batch) x (D + 1) entries, L.cap >= E.
int crf_build_lattice_features(int D, const CrfLattice& L, const PostDesc* d_imgs, const PostDesc* h_imgs, const float* d_feat, int B,
                               size_t ent_total, int max_pixels, const CrfBuildScratch& scratch, int* h_range_err, int* h_points, hipStream_t s);
int crf_feature_key_limit(int D);
int crf_lattice_norm(const CrfLattice& L, const PostDesc* d_imgs, int B, int max_pixels, size_t ent_total, float* va, float* vb,
                     float* norm_out, hipStream_t s);
// crf_meanfield.hip: the forward mean-field
// lattice(norm * Q): splat and the d + 1 blur axes; *result = the buffer that holds the filtered values (va or vb).  reverse:
// lattice^T(norm * Q), the blur axes in reverse order (the adjoint of the filter: the reverse mode's).  splat_only: no blur axes,
// *result = the splatted rows (pnp_crf_probe_filter)
int crf_filter(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* Q,
               float* va, float* vb, const float** result, int max_kp, hipStream_t s, bool reverse = false, bool splat_only = false);
// label output of the LAST mean-field update (argmax over the marginals it has just normalised, np.argmax semantics, remapped
// through the per-image LUT): lab[g] = label map of channel group g, null = no labels from this launch
struct CrfLabelOut {
    uint8_t* lab[2] = {nullptr, nullptr};
    const int32_t* lut = nullptr;
    int lut_stride = 0;
    const size_t* label_off = nullptr;
};
int crf_update(const CrfLattice& Lg, const CrfLattice& Lb, const PostDesc* d_imgs, int img0, int nimg, const float* vg,
               const float* vb, const float* norm_g, const float* norm_b, const float* unary, float* Q, float w_g,
               float w_b, int pairwise, int max_kp, int groups, hipStream_t s, const CrfLabelOut& labels = CrfLabelOut());
// The update with label-compatibility matrices (one channel group): Q <- softmax(-U + Mg msg_g + Mb msg_b).  The K x K message
// weights come TRANSPOSED in device memory, MgT[k * ldm + l] = Mg[l][k], ldm >= max_kp a multiple of 8, zeros wherever l or k is
// not a label.  kl_pix non-null: no update; the per-pixel terms of the KL divergence at the current Q (pnp_crf_kl) go to
// kl_pix[pixel of the batch].  crf_compat_tile_pixels: the tile it picks.
int crf_compat_tile_pixels(int max_kp, bool kl);
int crf_update_compat(const CrfLattice& Lg, const CrfLattice& Lb, const PostDesc* d_imgs, int img0, int nimg, const float* vg,
                      const float* vb, const float* norm_g, const float* norm_b, const float* unary, float* Q, const float* MgT,
                      const float* MbT, int ldm, int max_kp, hipStream_t s, const CrfLabelOut& labels, double* kl_pix);
// One pairwise term of a T-term update over caller-supplied features: row = (first ? -U : row) + compat(msg_t), and after the
// last term Q = softmax(row) with the label output.  L: the term's lattice (D1 = 2 .. 7); d_imgs: the term's descriptors
// (voff[0] = its value rows); val: what crf_filter left; base: unary rows (first) or logit rows; out: logit rows, or Q (last);
// base == out is allowed.  MT: K x K message weights transposed as crf_update_compat takes them, else wvec: one weight per
// label (ldm floats, zero beyond K), else the scalar w.
int crf_term_update(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* val, const float* norm, const float* base,
                    bool first, float* out, bool last, float w, const float* wvec, const float* MT, int ldm, int max_kp, hipStream_t s,
                    const CrfLabelOut& labels);
// crf_grad.hip: reverse mode of the T-term update (the sequence is crf_meanfield_backward of crf_solver.h)
// dl = Q (.) (g - <g, Q>) per pixel; gU -= dl.  Rows as Q
int crf_softmax_backward(const PostDesc* d_imgs, int img0, int nimg, const float* Q, const float* g, float* dl, float* gU, int max_pixels,
                         int max_kp, hipStream_t s);
// The tile of crf_term_backward (pixels, LDS bytes) for rows of up to max_kp floats, and the tiles of an H x W image
int crf_backward_tile_pixels(int max_kp, size_t* smem);
int crf_backward_tiles(int H, int W, int tile_pixels);
// h = C^T dl for one term (MT / wvec / w as crf_term_update).  val non-null -- the term's forward-filtered values of the update's
// input marginals -- : also one fp32 partial of psz floats (1, K or K * K) of the compatibility gradient per tile, at
// part[(tile0[b] - tile0[img0] + tile - t_lo) * psz]; tile0: [images of the batch + 1] first tile of every image (device).
// The launch takes the tiles [t_lo, t_hi) of every image: (0, INT_MAX) for whole images, else a span of ONE image (nimg = 1)
int crf_term_backward(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* val, const float* norm, const float* dl,
                      float* h, float w, const float* wvec, const float* MT, int ldm, int max_kp, float* part, const int* tile0, int psz,
                      int t_lo, int t_hi, hipStream_t s);
// The partials of images [img0, img0 + nimg), tiles [t_lo, t_hi) as above, in fp64: tiles in order within an image into img_sum
// (nimg x psz; continued from what it holds if t_lo > 0), and once an image's last span is in (`done`) acc[0 .. psz) += the
// images in order
int crf_grad_reduce(const float* part, const int* tile0, int img0, int nimg, int psz, double* img_sum, double* acc, int t_lo, int t_hi,
                    bool done, hipStream_t s);
int crf_grad_emit(const double* acc, int n, float* out, hipStream_t s);
// g (+)= norm * alpha * slice(val): a store when `first`
int crf_slice_add(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* val, const float* norm, float* g, bool first,
                  hipStream_t s);

}  // namespace pnp
