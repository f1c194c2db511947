// The entry points of include/pnp_hip.h that need no engine state of their own: the operator forms of this directory's kernels
// (pnp_op_*: what the tests and tools call one launch at a time), the stateless pipeline stages (ITC similarity, image
// preprocessing, JPEG decode) and the process-wide tuning / debug switches.  Argument checks and one launch each.
#include <cstring>

#include "engine.h"

using namespace pnp;

// sim = image_feat @ text_feat.t() (B/blip_image_text_matching.py:265).  Stateless.
extern "C" int pnp_itc_similarity(const float* d_img_feat, const float* d_txt_feat, int32_t B, int32_t T, int32_t E, float* d_sim,
                                  void* stream) {
    if (!d_img_feat || !d_txt_feat || !d_sim || B <= 0 || T <= 0 || E <= 0 || E % 4) return PNP_ERR_ARG;
    return itc_similarity(d_img_feat, d_txt_feat, d_sim, B, T, E, (hipStream_t)stream);
}

// The GemmArgs of an operator entry: every field an entry can set, in pnp_op_gemm_args' order with the split forms' low parts beside
// their high parts.  No checks: each entry keeps its own.
static GemmArgs gemm_op_args(const void* A, const void* A_lo, int lda, const void* B, const void* B_lo, int ldb, int M, int N, int K,
                             const float* bias, int bias_on_rows, const float* resid, int ldr, float* out_f32, int ldo, void* out_t,
                             void* out_lo, int ldo_t, int mode, float* aux, int ld_aux, int row_div, int col_div, int col_pad) {
    GemmArgs g = G_(A, lda, B, ldb, M, N, K);
    g.A_lo = A_lo; g.B_lo = B_lo;
    g.bias = bias; g.bias_on_rows = bias_on_rows; g.resid = resid; g.ldr = ldr;
    g.out_f32 = out_f32; g.ldo = ldo; g.out_t = out_t; g.out_lo = out_lo; g.ldo_t = ldo_t;
    g.mode = mode; g.aux = aux; g.ld_aux = ld_aux; g.row_div = row_div; g.col_div = col_div; g.col_pad = col_pad;
    return g;
}

extern "C" int pnp_op_gemm_ex(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                              int32_t K, const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo,
                              void* d_out_t, int32_t ldo_t, int32_t mode, void* stream) {
    return gemm_nt(bf, gemm_op_args(d_A, nullptr, lda, d_B, nullptr, ldb, M, N, K, d_bias, 0, d_resid, ldr, d_out_f32, ldo, d_out_t, nullptr, ldo_t,
                                    mode ? GEMM_EPI_GELU : GEMM_EPI_LINEAR, nullptr, 0, 0, 0, 0), (hipStream_t)stream);
}

extern "C" int pnp_op_gemm(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                           int32_t K, const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo,
                           int32_t gelu, void* stream) {
    return pnp_op_gemm_ex(bf, d_A, lda, d_B, ldb, M, N, K, d_bias, d_resid, ldr, d_out_f32, ldo, nullptr, 0, gelu, stream);
}

extern "C" int pnp_op_split(const float* d_in, void* d_hi, void* d_lo, int64_t n, void* stream) {
    if (!d_in || !d_hi || !d_lo || n <= 0) return PNP_ERR_ARG;
    return split_f32(d_in, d_hi, d_lo, (size_t)n, (hipStream_t)stream);
}

extern "C" int pnp_op_gemm_x3(const void* d_A_hi, const void* d_A_lo, int32_t lda, const void* d_B_hi, const void* d_B_lo,
                              int32_t ldb, int32_t M, int32_t N, int32_t K, const float* d_bias, int32_t bias_on_rows,
                              const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo, void* d_out_hi, void* d_out_lo,
                              int32_t ldo_t, int32_t gelu, int32_t col_div, int32_t col_pad, void* stream) {
    if (!d_A_hi || !d_A_lo || !d_B_hi || !d_B_lo) return PNP_ERR_ARG;
    GemmArgs g = gemm_op_args(d_A_hi, d_A_lo, lda, d_B_hi, d_B_lo, ldb, M, N, K, d_bias, bias_on_rows, d_resid, ldr, d_out_f32, ldo, d_out_hi,
                              d_out_lo, ldo_t, gelu ? GEMM_EPI_GELU : GEMM_EPI_LINEAR, nullptr, 0, 0, col_div, col_pad);
    g.sk = streamk_mode() ? streamk_ws_default() : nullptr;     // op level: the per-device workspace (shared by all callers: the launcher serialises)
    return gemm_nt(1, g, (hipStream_t)stream);
}

extern "C" int pnp_set_tuning(const char* key, int32_t value) {
    if (!key) return PNP_ERR_ARG;
    if (!strcmp(key, "streamk")) {
        if (value < 0 || value > 2) return PNP_ERR_ARG;
        set_streamk_mode(value);
        return PNP_OK;
    }
    if (!strcmp(key, "text_rows")) {
        if (value < 0 || value > 4) return PNP_ERR_ARG;
        set_text_rows(value);
        return PNP_OK;
    }
    if (!strcmp(key, "gemm_stamps")) {
        if (value < 0 || value > 1) return PNP_ERR_ARG;
        return gemm_set_stamps(value);
    }
    return PNP_ERR_ARG;
}

extern "C" int pnp_streamk_status(pnp_engine* e, int64_t* launches, uint32_t* gave_up) {
    if (!launches || !gave_up) return PNP_ERR_ARG;
    StreamKWs* ws = e ? &e->sk_ws : streamk_ws_default();
    *launches = ws ? ws->launches : 0;
    *gave_up = 0;
    if (!ws || !ws->part) return PNP_OK;
    if (e) HIPCHK(e, hipSetDevice(e->c.device));
    if (hipDeviceSynchronize() != hipSuccess) return PNP_ERR_HIP;
    return streamk_ws_timeouts(ws, gave_up);
}

extern "C" int pnp_op_gemm_x3a(const float* d_A, int32_t lda, const void* d_B_hi, const void* d_B_lo, int32_t ldb, int32_t M,
                               int32_t N, int32_t K, const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32,
                               int32_t ldo, int32_t mode, float* d_aux, int32_t ld_aux, void* stream) {
    if (!d_A || !d_B_hi || !d_B_lo || !d_out_f32 || mode < 0 || mode > 2) return PNP_ERR_ARG;
    GemmArgs g = gemm_op_args(d_A, nullptr, lda, d_B_hi, d_B_lo, ldb, M, N, K, d_bias, 0, d_resid, ldr, d_out_f32, ldo, nullptr, nullptr, 0, mode,
                              d_aux, ld_aux, 0, 0, 0);
    g.a_f32 = 1;
    return gemm_nt(0, g, (hipStream_t)stream);
}

extern "C" int pnp_op_gemm_tokcols(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                                   int32_t K, const float* d_bias_rows, void* d_out_t, int32_t ldo_t, int32_t col_div,
                                   int32_t col_pad, void* stream) {
    if (!d_out_t || col_div < 0 || (col_div > 0 && col_pad < col_div)) return PNP_ERR_ARG;
    return gemm_nt(bf, gemm_op_args(d_A, nullptr, lda, d_B, nullptr, ldb, M, N, K, d_bias_rows, 1, nullptr, 0, nullptr, 0, d_out_t, nullptr, ldo_t,
                                    GEMM_EPI_LINEAR, nullptr, 0, 0, col_div, col_pad), (hipStream_t)stream);
}

extern "C" int pnp_op_gemm_args(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                                int32_t K, const float* d_bias, int32_t bias_on_rows, const float* d_resid, int32_t ldr,
                                float* d_out_f32, int32_t ldo, void* d_out_t, int32_t ldo_t, int32_t mode, float* d_aux,
                                int32_t ld_aux, int32_t row_div, int32_t col_div, int32_t col_pad, void* stream) {
    if (!d_A || !d_B || (!d_out_f32 && !d_out_t) || M <= 0 || N <= 0 || K <= 0 || lda < K || ldb < K) return PNP_ERR_ARG;
    if (mode < 0 || mode > 2 || (mode == GEMM_EPI_GELU_GRAD && !d_aux)) return PNP_ERR_ARG;
    if (row_div < 0 || col_div < 0 || (col_div > 0 && col_pad < col_div)) return PNP_ERR_ARG;
    return gemm_nt(bf ? 1 : 0, gemm_op_args(d_A, nullptr, lda, d_B, nullptr, ldb, M, N, K, d_bias, bias_on_rows ? 1 : 0, d_resid, ldr, d_out_f32, ldo,
                                            d_out_t, nullptr, ldo_t, mode, d_aux, ld_aux, row_div, col_div, col_pad), (hipStream_t)stream);
}

// The launch plan of the entry points above (include/pnp_hip.h): the same GemmArgs with a placeholder for every pointer that is
// present -- gemm_plan looks at which are set, never at what they hold.  The wide split form needs both low parts, the text-side
// form the weight's.
extern "C" int pnp_op_gemm_plan(int32_t form, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t mode, int32_t has,
                                int32_t row_div, int32_t col_div, int32_t col_pad, int32_t n_cu, int32_t streamk_mode, int32_t sk_wgs,
                                pnp_gemm_plan* plan) {
    if (!plan || form < PNP_GEMM_FORM_F32 || form > PNP_GEMM_FORM_X3A) return PNP_ERR_ARG;
    static float there[4];
    auto p = [&](int bit) { return (has & bit) ? there : nullptr; };
    const bool x3 = form == PNP_GEMM_FORM_X3, x3a = form == PNP_GEMM_FORM_X3A;
    GemmArgs g = gemm_op_args(there, x3 ? there : nullptr, lda, there, x3 || x3a ? there : nullptr, ldb, M, N, K, p(PNP_GEMM_HAS_BIAS),
                              (has & PNP_GEMM_HAS_BIAS_ON_ROWS) ? 1 : 0, p(PNP_GEMM_HAS_RESID), 0, p(PNP_GEMM_HAS_OUT_F32), 0, p(PNP_GEMM_HAS_OUT_T),
                              p(PNP_GEMM_HAS_OUT_LO), 0, mode, p(PNP_GEMM_HAS_AUX), 0, row_div, col_div, col_pad);
    g.a_f32 = x3a;
    *plan = gemm_plan(form == PNP_GEMM_FORM_BF16 || x3, g, n_cu, streamk_mode, sk_wgs);
    return plan->status;
}

extern "C" int pnp_op_vit_attention(int32_t bf, const void* d_qk, int32_t ld_qk, int32_t D, const void* d_vt, int32_t ld_vt,
                                    int32_t n_pad, void* d_ctx, int32_t B, int32_t heads, int32_t N, float scale, void* stream) {
    if (!d_qk || !d_vt || !d_ctx || B <= 0 || heads <= 0 || N <= 0) return PNP_ERR_ARG;
    return vit_attention(bf, d_qk, ld_qk, D, d_vt, ld_vt, n_pad, d_ctx, B, heads, N, scale, (hipStream_t)stream);
}

extern "C" int pnp_op_vit_attention_x3(const void* d_qkv_hi, const void* d_qkv_lo, int32_t ld_qkv, int32_t D, void* d_ctx_hi,
                                       void* d_ctx_lo, int32_t B, int32_t heads, int32_t N, float scale, void* stream) {
    if (B <= 0 || heads <= 0 || N <= 0 || ld_qkv < 3 * D) return PNP_ERR_ARG;
    return vit_attention_x3(d_qkv_hi, d_qkv_lo, ld_qkv, D, d_ctx_hi, d_ctx_lo, B, heads, N, scale, (hipStream_t)stream);
}

extern "C" int pnp_op_layernorm(const float* d_x, const float* d_w, const float* d_b, float eps, int32_t rows, int32_t D,
                                float* d_y, void* stream) {
    return layernorm(0, d_x, d_w, d_b, eps, rows, D, d_y, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int pnp_op_xattn(int32_t bf16, int32_t mode, const void* d_nat, int32_t ld_nat, const void* d_tr, int32_t ld_tr,
                            int32_t n_pad, const void* d_x, int32_t ldx, void* d_out, int32_t ldo, float* d_probs,
                            int32_t n_stride, int32_t B, int32_t L, int32_t N, int32_t heads, void* stream) {
    if (!d_nat || !d_x || !d_probs || mode < 0 || mode > 2 || (mode != 2 && (!d_tr || !d_out))) return PNP_ERR_ARG;
    if (B <= 0 || L <= 0 || N <= 0 || heads <= 0) return PNP_ERR_ARG;
    return xattn(bf16, mode, d_nat, ld_nat, d_tr, ld_tr, n_pad, d_x, ldx, d_out, ldo, d_probs, n_stride, B, L, N, heads,
                 (hipStream_t)stream);
}

extern "C" int pnp_op_text_self_attn(int32_t bf16, const void* d_qkv, const int64_t* d_mask, int32_t ld_mask, void* d_ctx,
                                     float* d_probs, float* d_scratch, int32_t B, int32_t L, int32_t H, void* stream) {
    if (!d_qkv || !d_mask || !d_ctx || B <= 0 || L <= 0 || H <= 0 || ld_mask < L) return PNP_ERR_ARG;
    return text_self_attn(bf16, d_qkv, d_mask, ld_mask, d_ctx, d_probs, d_scratch, B, L, H, (hipStream_t)stream);
}

extern "C" int pnp_op_text_self_attn_bwd(int32_t bf16, const void* d_qkv, const float* d_dctx, const float* d_probs,
                                         float* d_ds_scratch, void* d_dqkv, int32_t B, int32_t L, int32_t H, void* stream) {
    if (!d_qkv || !d_dctx || !d_probs || !d_ds_scratch || !d_dqkv || B <= 0 || L <= 0 || H <= 0) return PNP_ERR_ARG;
    return text_self_attn_bwd(bf16, d_qkv, d_dctx, d_probs, d_ds_scratch, d_dqkv, B, L, H, (hipStream_t)stream);
}

extern "C" int pnp_op_layernorm_ex(int32_t bf16, const float* d_x, const float* d_w, const float* d_b, float eps, int32_t rows,
                                   int32_t D, float* d_y, void* d_yt, void* d_yt_lo, float* d_xhat, float* d_rstd, void* stream) {
    if (!d_x || !d_w || !d_b || rows <= 0 || D <= 0 || (d_yt_lo && !d_yt)) return PNP_ERR_ARG;
    return layernorm(bf16, d_x, d_w, d_b, eps, rows, D, d_y, d_yt, d_xhat, d_rstd, (hipStream_t)stream, d_yt_lo);
}

extern "C" int pnp_op_layernorm_bwd(int32_t bf16, const float* d_dy, const float* d_w, const float* d_xhat, const float* d_rstd,
                                    int32_t rows, int32_t D, float* d_dx, void* d_dxt, void* stream) {
    if (!d_dy || !d_w || !d_xhat || !d_rstd || rows <= 0 || D <= 0) return PNP_ERR_ARG;
    return layernorm_bwd(bf16, d_dy, d_w, d_xhat, d_rstd, rows, D, d_dx, d_dxt, (hipStream_t)stream);
}

extern "C" int pnp_op_text_embed(const int64_t* d_ids, int32_t ld_ids, const float* d_word, const float* d_pos, float* d_out,
                                 int32_t B, int32_t L, int32_t H, int32_t enc_id, int32_t vocab, void* stream) {
    if (!d_ids || !d_word || !d_pos || !d_out || B <= 0 || L <= 0 || H <= 0 || H % 4 || vocab <= 0 || ld_ids < L || enc_id >= vocab)
        return PNP_ERR_ARG;
    return text_embed(d_ids, ld_ids, d_word, d_pos, d_out, B, L, H, enc_id, vocab, (hipStream_t)stream);
}

extern "C" int pnp_op_itm_head(const float* d_hlast, const float* d_w, const float* d_bias, float* d_logits, int32_t B, int32_t L,
                               int32_t H, void* stream) {
    if (!d_hlast || !d_w || !d_bias || !d_logits || B <= 0 || L <= 0 || H <= 0) return PNP_ERR_ARG;
    return itm_head(d_hlast, d_w, d_bias, d_logits, B, L, H, (hipStream_t)stream);
}

extern "C" int pnp_op_itm_grad_seed(const float* d_w, float* d_dh, int32_t B, int32_t L, int32_t H, void* stream) {
    if (!d_w || !d_dh || B <= 0 || L <= 0 || H <= 0) return PNP_ERR_ARG;
    return itm_grad_seed(d_w, d_dh, B, L, H, (hipStream_t)stream);
}

extern "C" int pnp_op_patchify(int32_t bf16, const float* d_img, const uint8_t* d_dropped, void* d_out, int32_t B, int32_t S,
                               int32_t P, void* stream) {
    if (!d_img || !d_out || B <= 0 || P <= 0 || S != P * 16) return PNP_ERR_ARG;
    return patchify(bf16, d_img, d_dropped, d_out, B, S, P, (hipStream_t)stream);
}

extern "C" int pnp_op_cls_rows(const float* d_cls, const float* d_pos, float* d_x, int32_t B, int32_t N, int32_t D, void* stream) {
    if (!d_cls || !d_pos || !d_x || B <= 0 || N <= 0 || D <= 0) return PNP_ERR_ARG;
    return cls_rows(d_cls, d_pos, d_x, B, N, D, (hipStream_t)stream);
}

extern "C" int pnp_dbg_gemm_stamps(uint64_t* host_out, int32_t max_blocks) {
    return gemm_read_stamps((unsigned long long*)host_out, max_blocks);
}

extern "C" int pnp_preprocess_images(const uint8_t* d_rgb, const pnp_pre_image* d_desc, int32_t B, int32_t S, int32_t max_H,
                                     const int32_t* d_coef, uint8_t* d_tmp, const float* mean3, const float* std3,
                                     float* d_out, void* stream) {
    if (!d_rgb || !d_desc || !d_coef || !d_tmp || !mean3 || !std3 || !d_out) return PNP_ERR_ARG;
    static_assert(sizeof(pnp_pre_image) == 40, "pnp_pre_image layout is part of the ABI");
    return preprocess_images(d_rgb, d_desc, B, S, max_H, d_coef, d_tmp, mean3, std3, d_out, (hipStream_t)stream);
}

extern "C" int pnp_jpeg_decode(const uint8_t* d_data, const pnp_jpeg_image* d_images, const pnp_jpeg_tables* d_tables,
                               const pnp_jpeg_segment* d_segments, int32_t n_images, int32_t n_segments, uint8_t* d_clean,
                               int32_t* d_seg_bits, int16_t* d_coef, int64_t coef_elems, uint8_t* d_planes, uint8_t* d_rgb,
                               int32_t max_blocks_per_image, int32_t max_pixels_per_image, int32_t* d_err, void* stream) {
    if (!d_data || !d_images || !d_tables || !d_segments || !d_clean || !d_seg_bits || !d_coef || !d_planes || !d_rgb || !d_err ||
        coef_elems <= 0)
        return PNP_ERR_ARG;
    static_assert(sizeof(pnp_jpeg_image) == sizeof(JpegImage) && sizeof(pnp_jpeg_tables) == sizeof(JpegTables) &&
                      sizeof(pnp_jpeg_segment) == sizeof(JpegSegment), "JPEG descriptor layouts are part of the ABI");
    return jpeg_decode(d_data, reinterpret_cast<const JpegImage*>(d_images), reinterpret_cast<const JpegTables*>(d_tables),
                       reinterpret_cast<const JpegSegment*>(d_segments), n_images, n_segments, d_clean, d_seg_bits, d_coef,
                       (size_t)coef_elems, d_planes, d_rgb, max_blocks_per_image, max_pixels_per_image, d_err, (hipStream_t)stream);
}

extern "C" int pnp_jpeg_decode_scans(const uint8_t* d_data, const pnp_jpeg_image* d_images, const pnp_jpeg_tables* d_tables,
                                     const pnp_jpeg_scan* d_scans, const pnp_jpeg_segment* d_segments, int32_t n_images,
                                     int32_t n_scans, int32_t n_segments, int32_t n_base_segments, const int32_t* h_groups,
                                     int32_t n_groups, uint8_t* d_clean, int32_t* d_seg_bits, int16_t* d_coef, int64_t coef_elems,
                                     uint64_t* d_hist, uint8_t* d_planes, uint8_t* d_rgb, int32_t max_blocks_per_image,
                                     int32_t max_pixels_per_image, int32_t* d_rounds, float* h_group_ms, int32_t* d_err, void* stream) {
    if (!d_data || !d_images || !d_tables || !d_scans || !d_segments || !d_clean || !d_seg_bits || !d_coef || !d_planes || !d_rgb ||
        !d_err || coef_elems <= 0 || coef_elems % 64)
        return PNP_ERR_ARG;
    if (n_images <= 0 || n_scans < n_images || n_segments < n_scans || n_base_segments < 0 || n_base_segments > n_segments ||
        n_groups < 0 || (n_groups > 0 && !h_groups))
        return PNP_ERR_ARG;
    int next = n_base_segments;                           // the groups tile the progressive segments, in order
    bool refine = false;
    for (int g = 0; g < n_groups; g++) {
        const int32_t* q = h_groups + 4 * g;
        if (q[0] != next || q[1] <= 0 || q[1] > n_segments - next || q[2] < 1 || q[2] > 4 || q[3] < 0) return PNP_ERR_ARG;
        if (g > 0 && (q[3] < q[-1] || (q[3] == q[-1] && q[2] <= q[-2]))) return PNP_ERR_ARG;
        refine = refine || q[2] == 4;
        next += q[1];
    }
    if (next != n_segments || (refine && !d_hist)) return PNP_ERR_ARG;
    static_assert(sizeof(pnp_jpeg_scan) == sizeof(JpegScan) && sizeof(pnp_jpeg_segment) == sizeof(JpegSegment),
                  "JPEG descriptor layouts are part of the ABI");
    return jpeg_decode_scans(d_data, reinterpret_cast<const JpegImage*>(d_images), reinterpret_cast<const JpegTables*>(d_tables),
                             reinterpret_cast<const JpegScan*>(d_scans), reinterpret_cast<const JpegSegment*>(d_segments), n_images,
                             n_segments, n_base_segments, h_groups, n_groups, d_clean, d_seg_bits, d_coef, (size_t)coef_elems, d_hist,
                             d_planes, d_rgb, max_blocks_per_image, max_pixels_per_image, d_rounds, h_group_ms, d_err, (hipStream_t)stream);
}

// operator forms of the lattice build's sort / scan (tests); the scratch is allocated per call
extern "C" int pnp_op_sort_pairs(uint64_t* d_keys_in, uint64_t* d_keys_out, uint32_t* d_vals_in, uint32_t* d_vals_out, int64_t n,
                                 int32_t begin_bit, int32_t end_bit, const size_t* h_seg_off, int32_t n_seg, void* stream) {
    if (n < 0 || (n && (!d_keys_in || !d_keys_out || !d_vals_in || !d_vals_out))) return PNP_ERR_ARG;
    if (!n) return PNP_OK;
    const size_t tb = sort_temp_bytes((size_t)n);
    void* temp = nullptr;
    if (hipMalloc(&temp, tb) != hipSuccess) return PNP_ERR_NOMEM;
    int r = radix_sort_pairs(d_keys_in, d_keys_out, d_vals_in, d_vals_out, (size_t)n, begin_bit, end_bit, h_seg_off, n_seg, temp, tb, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && r == PNP_OK) r = PNP_ERR_HIP;
    (void)hipFree(temp);
    return r;
}
extern "C" int pnp_op_scan_i32(const int32_t* d_in, int32_t* d_out, int64_t n, int32_t inclusive, void* stream) {
    if (n < 0 || (n && (!d_in || !d_out))) return PNP_ERR_ARG;
    if (!n) return PNP_OK;
    const size_t tb = sort_temp_bytes((size_t)n);
    void* temp = nullptr;
    if (hipMalloc(&temp, tb) != hipSuccess) return PNP_ERR_NOMEM;
    int r = device_scan_i32(d_in, d_out, (size_t)n, inclusive != 0, temp, tb, (hipStream_t)stream);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && r == PNP_OK) r = PNP_ERR_HIP;
    (void)hipFree(temp);
    return r;
}

extern "C" int pnp_op_cast(int32_t to_bf16, const float* d_in, void* d_out, int64_t n, void* stream) {
    return cast_f32(to_bf16, d_in, d_out, (size_t)n, (hipStream_t)stream);
}
