/* pnp_hip.h -- C ABI of libpnp_hip.so, the MI355X (gfx950) engine behind the PnP-OVSS hot path.
 *
 * The reference (letitiabanana/PnP-OVSS) is pure Python and has NO native boundary of its own; the
 * closest analogue is pydensecrf's DenseCRF2D object (PnP_OVSS_0514_updated_segmentation.py:
 * 1066-1071).  Each entry point below therefore cites the reference *Python* interface it replaces
 * (PnP.py = PnP_OVSS_0514_updated_segmentation.py, B/ = "Files to replace for BLIP/").
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types; every call returns 0 or a negative
 *     errno-style code, message via pnp_last_error(); no exception crosses the boundary.
 *   - "d_" pointers are DEVICE pointers owned by the caller (e.g. torch tensor .data_ptr()),
 *     contiguous row-major; `stream` is a hipStream_t (NULL = default stream).
 *   - All device memory the engine needs is allocated in pnp_create / pnp_post_reserve; the hot
 *     path calls allocate nothing and never synchronise the device (hipGraph-capturable) except
 *     where stated.
 *   - One process per device (PnP.py:1439).  An engine is not thread-safe: calls on one engine must not overlap.  Distinct
 *     engines of a process are independent (own workspace, caller's stream) and may be driven concurrently from different
 *     host threads: that is how a host keeps several batches in flight on one GPU (bench.py --pipelines, the CLI's
 *     --pipelines; tests/test_hip_parity.py::test_engines_in_flight_match_one_at_a_time).
 */
#ifndef PNP_HIP_H
#define PNP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pnp_engine pnp_engine;

/* Geometry of `load_model_and_preprocess("blip_image_text_matching", "large")`
 * (B/blip_itm_large.yaml, B/vit.py:511-523, LAVIS med_large_config.json). */
typedef struct pnp_config {
    int32_t img_size, patch, vit_dim, vit_depth, vit_heads, vit_mlp_ratio;
    float vit_ln_eps;
    int32_t txt_hidden, txt_layers, txt_heads, txt_inter;
    float txt_ln_eps;
    int32_t vocab, max_pos, enc_token_id;
    int32_t max_batch;      /* images per step (--batch_size, PnP.py:58) */
    int32_t max_text_len;   /* longest tokenised caption the engine must hold (<= 512 = BERT's position table; the reference
                             * tokenises to max_length 500, PnP.py:271,318) */
    int32_t stash_layer;    /* args.max_att_block_num - 1 (PnP.py:619): text layer whose P and dL/dP are kept */
    int32_t compute_bf16;   /* arithmetic of the dense contractions:
                             *   0  exact fp32 MFMA everywhere (the reference's arithmetic; parity mode)
                             *   1  bf16 storage + bf16 MFMA with fp32 accumulation (throughput mode; ~1 % error on image_embeds)
                             *   2  split-bf16 ("bf16x3", the benchmarked mode): EVERY dense contraction of the model -- the ViT Linears and
                             *      the ViT self-attention, the cross K/V projections, the text-side Linears and their analytic
                             *      backward -- on (hi, lo) bf16 operand pairs, three bf16 MFMA passes per product with fp32
                             *      accumulation: fp32-class results (maps within 1e-4 of mode 0, same patch picks) at ~5x the
                             *      fp32 MFMA rate.  Softmax, LayerNorm, the text self- / cross-attention kernels (fp32 operands)
                             *      and all post-processing are the mode-0 code */
    int32_t device;         /* HIP device ordinal */
} pnp_config;

/* ---- lifetime ---------------------------------------------------------------------------- */
int pnp_create(const pnp_config* cfg, pnp_engine** out);
/* A second engine on the donor's WEIGHTS (same device, compute mode and model geometry; cfg->stash_layer >= the donor's;
 * max_batch / max_text_len free): allocates activations and workspace only, never calls pnp_load_weight /
 * pnp_finalize_weights, and keeps the weights alive past the donor's pnp_destroy (shared ownership).  What `--pipelines P`
 * / bench.py's batches in flight run on: P engines, one weight copy (the reference holds one replica per process,
 * PnP.py:1212-1218; several batches in flight per GPU are this build's addition). */
int pnp_create_shared(const pnp_config* cfg, pnp_engine* donor, pnp_engine** out);
void pnp_destroy(pnp_engine* e);
const char* pnp_last_error(const pnp_engine* e);          /* valid until the next call on e */
size_t pnp_workspace_bytes(const pnp_config* cfg);         /* device bytes pnp_create will allocate */
size_t pnp_allocated_bytes(const pnp_engine* e);           /* device bytes the engine holds now (create + post_reserve + weights) */

/* Weights in: replaces BaseModel.load_checkpoint + load_state_dict (B/base_model.py:86-125).
 * `name` is the reference state-dict key ("visual_encoder.blocks.3.attn.qkv.weight", ...), data is
 * fp32 (host pointer, or device pointer when on_device != 0, e.g. after an RCCL broadcast).
 * Unknown names are ignored (strict=False), shape mismatches are errors. */
int pnp_load_weight(pnp_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim,
                    int32_t on_device);
/* Builds fused / transposed device copies; fails with the first missing tensor name. Synchronises. */
int pnp_finalize_weights(pnp_engine* e);

/* ---- model: replaces BlipITM.forward(match_head="itm") + loss.backward() + hooks -------- */
/* VisionTransformer.forward (B/vit.py:274-290).  d_images: (B,3,S,S) fp32 normalised.
 * d_dropped: optional (B, P*P) uint8, 1 = patch zeroed by the salience drop (PnP.py:597-603). */
int pnp_vit_forward(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, int32_t B, void* stream);
/* key / value Linear(1024 -> 768) of every text layer's cross-attention applied to image_embeds (B/med.py:208-211,
 * encoder_hidden_states branch), all layers at once.  pnp_vit_forward ends with this call; it is exported on its own
 * so the projections can be re-run on the engine's current image_embeds (precision probes, tests). */
int pnp_cross_kv(pnp_engine* e, int32_t B, void* stream);
/* BertModel.forward(mode="multimodal") + itm_head (B/med.py:854-1024, B/blip_image_text_matching.py:
 * 238-249); stashes the cross-attention probabilities of layers >= stash_layer (B/med.py:280-283).
 * d_ids / d_mask: (B, ld) int64, the first L columns are used (padding="longest").  Ids outside [0, vocab) are clamped to
 * the nearest valid id; a caption whose mask is all zeros gives finite results (see pnp_op_text_self_attn). */
int pnp_text_forward_xattn(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t B,
                           int32_t L, float* d_logits, void* stream);
/* loss = logits[:,1].sum(); loss.backward() restricted to what reaches attention_probs of
 * stash_layer (B/blip_image_text_matching.py:399-404, hook B/med.py:164-168). */
int pnp_xattn_grad(pnp_engine* e, int32_t B, int32_t L, void* stream);
/* The same backward stopped at any kept layer (stash_layer <= layer < txt_layers): after it "P" / "dP" and
 * pnp_gradcam_gather refer to that layer.  With stash_layer = 0 every [layer][head] entry of compute_gradcam_ensemble's
 * return value (B/blip_image_text_matching.py:411-435; the drivers' --ensemble_blocks / layer-head sweep reads them) is
 * available from one forward: one pnp_xattn_grad_layer + 12 gathers per layer. */
int pnp_xattn_grad_layer(pnp_engine* e, int32_t B, int32_t L, int32_t layer, void* stream);
/* cams * relu(grads) * mask for one head, [ENC] row and image-CLS column dropped
 * (B/blip_image_text_matching.py:427-433).  d_out: (B, L-1, P, P) fp32. */
int pnp_gradcam_gather(pnp_engine* e, const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t head,
                       float* d_out, void* stream);
/* compute_gradcam_ensemble for [stash_layer][head] (B/blip_image_text_matching.py:386-457). */
int pnp_compute_gradcam(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, const int64_t* d_ids,
                        const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t head, float* d_out,
                        float* d_logits, void* stream);

/* ... for [layer][head], stash_layer <= layer (args.max_att_block_num - 1 chosen per call: layer / head sweeps). */
int pnp_compute_gradcam_layer(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, const int64_t* d_ids,
                              const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t layer, int32_t head,
                              float* d_out, float* d_logits, void* stream);

/* ---- ITC head and feature extraction: replaces BlipITM.forward(match_head="itc") and BlipITM.extract_features
 * (B/blip_image_text_matching.py:253-266, 59-189).  They need the optional weights vision_proj.weight / .bias (E, vit_dim) and
 * text_proj.weight / .bias (E, txt_hidden), E = the weight's first dimension (256 in every BLIP config, a multiple of 64):
 * pnp_finalize_weights succeeds without them, pnp_project_normalize then returns PNP_ERR_STATE naming the missing tensor.
 * Engines made by pnp_create_shared use the donor's copy. */
/* BertModel.forward(mode="text") (B/med.py:565-568, 473): the text stack with self-attention and feed-forward only -- no
 * cross-attention, token 0 kept as given (no [ENC] substitution) -- for T texts of L tokens, 2 <= L <= max_text_len, that need
 * no image: T may exceed max_batch (e.g. 150 class prompts), the call then works through max_batch rows of text at a time, and
 * a row's result does not depend on T.  d_ids / d_mask: (T, ld) int64, the first L columns are used.  d_hidden: (T, L, H)
 * fp32 last_hidden_state, or NULL (the last max_batch-row piece stays readable as "text_hidden").  Runs in the activation
 * buffers of pnp_text_forward_xattn: afterwards pnp_xattn_grad* / pnp_gradcam_gather fail (PNP_ERR_STATE) until the next
 * multimodal forward; image_embeds and the cross-attention keys / values of the last pnp_vit_forward stay as they are. */
int pnp_text_forward_text(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t T, int32_t L,
                          float* d_hidden, void* stream);
/* F.normalize(proj(x), dim=-1), proj = vision_proj (which = 0, K = vit_dim) or text_proj (which = 1, K = txt_hidden)
 * (B/blip_image_text_matching.py:137-138, 158-159, 260-263): d_out[r, :] = y / max(||y||_2, 1e-12), y = W . x_r + b.
 * d_x: fp32, row r at d_x + r * row_stride (row_stride >= K elements, a multiple of 4; rows * row_stride * 4 < 4 GiB) -- the CLS
 * rows of a (B, N, D) tensor are row_stride = N * D, rows = B, no gather.  d_out: (rows, E) fp32.  The Linear runs in the
 * engine's compute mode (exact fp32 MFMA | split-bf16 | bf16), the normalisation in fp32. */
int pnp_project_normalize(pnp_engine* e, int32_t which, const float* d_x, int64_t row_stride, int32_t rows, float* d_out,
                          void* stream);
/* sim = image_feat @ text_feat.t() (B/blip_image_text_matching.py:265): d_sim[b, t] = sum_e d_img_feat[b, e] * d_txt_feat[t, e],
 * plain fp32 FMA in a fixed order (independent of the compute mode).  E a multiple of 4.  Stateless. */
int pnp_itc_similarity(const float* d_img_feat, const float* d_txt_feat, int32_t B, int32_t T, int32_t E, float* d_sim,
                       void* stream);

/* ---- salience-drop loop: replaces Inference_BLIP_filteredcaption (PnP.py:564-722) -------- */
/* One bookkeeping step (PnP.py:619-647 + the running sum of :716-721) on a gathered map. */
int pnp_drop_step(pnp_engine* e, const float* d_gradcam, float* d_g0, float* d_agg, uint8_t* d_dropped,
                  int32_t* d_picks, int32_t iter, int32_t B, int32_t T, int32_t npick, int32_t max_picks,
                  void* stream);
/* The whole loop, device resident, no host sync.  d_g0 / d_agg: (B, L-1, P, P); d_picks: (B, drop_iter*npick)
 * int32 patch ids in pick order; drop_iter == 1 -> single forward, d_agg untouched. */
int pnp_drop_loop(pnp_engine* e, const float* d_images, const int64_t* d_ids, const int64_t* d_mask, int32_t ld,
                  int32_t B, int32_t L, int32_t head, int32_t drop_iter, int32_t npick, float* d_g0, float* d_agg,
                  int32_t* d_picks, float* d_logits, void* stream);

/* The loop on the maps of another kept text layer (stash_layer <= layer). */
int pnp_drop_loop_layer(pnp_engine* e, const float* d_images, const int64_t* d_ids, const int64_t* d_mask, int32_t ld,
                        int32_t B, int32_t L, int32_t layer, int32_t head, int32_t drop_iter, int32_t npick, float* d_g0,
                        float* d_agg, int32_t* d_picks, float* d_logits, void* stream);

/* ---- post-process: replaces PnP.py:348-403 / 424-481 + postprocess/densecrf/scores ------ */
typedef struct pnp_post_batch {
    int32_t B;
    const int32_t* H;            /* [B] original image height (label_trues[img].shape[0]) */
    const int32_t* W;            /* [B] */
    const int32_t* n_classes;    /* [B] selected classes (len(best_class_idx_list[img])) */
    const int32_t* has_bg;       /* [B] background channel prepended (PnP.py:373-379) */
    /* Mean_over_filtered_label_tokens plan (PnP.py:810-853): class c of image b sums tokens
     * tok_idx[cls_off[img_cls_off[b]+c] .. cls_off[img_cls_off[b]+c+1]) (indices into map[3:-1]),
     * then divides by cls_div when != 1 */
    const int32_t* img_cls_off;  /* [B+1] */
    const int32_t* cls_off;      /* [total_classes+1] */
    const int32_t* tok_idx;      /* [total_tokens] */
    const int32_t* cls_div;      /* [total_classes] */
    const int32_t* lut;          /* [B*lut_stride] argmax index -> dataset class id (PnP.py:390-399 folded) */
    int32_t lut_stride;
    const uint8_t* d_rgb;        /* device: concatenated original RGB images (sum H*W*3), CRF bilateral */
    const float* d_gt;           /* device: concatenated ground-truth label maps (sum H*W) or NULL */
    /* optional host-provided Gaussian taps (float64), image b uses blur_wts[blur_wt_off[b] + j] for
     * distance j = 0..radius, radius = blur_wt_off[b+1] - blur_wt_off[b] - 1.  NULL: computed by the
     * engine as scipy's _gaussian_kernel1d(0.05 * max(H, W), truncate 4).  The Python host passes
     * numpy-computed taps so the blur is bit-identical to scipy.ndimage.gaussian_filter. */
    const double* blur_wts;
    const int32_t* blur_wt_off;  /* [B+1] */
} pnp_post_batch;

/* Reserve device memory for post-processing batches up to these bounds (call once; allocates). */
int pnp_post_reserve(pnp_engine* e, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image,
                     int32_t max_channels, int32_t crf_chunk);
/* Upload descriptors/plan of a batch, compute blur taps, and (when want_crf) build both
 * permutohedral lattices + normalisers for its images.  Synchronises once (range check). */
int pnp_post_prepare(pnp_engine* e, const pnp_post_batch* batch, int32_t want_crf, void* stream);
/* Stage calls operate on the prepared batch and the engine's internal map buffers. */
int pnp_merge_tokens(pnp_engine* e, const float* d_gradcam, int32_t T, void* stream);          /* PnP.py:810-853 */
int pnp_threshold_upsample(pnp_engine* e, float threshold, int32_t scale01, void* stream);      /* PnP.py:348-379 */
int pnp_blur_minmax(pnp_engine* e, void* stream);                                               /* PnP.py:1149-1153 */
int pnp_densecrf(pnp_engine* e, int32_t iters, float pos_w, float pos_xy, float bi_w, float bi_xy, float bi_rgb,
                 void* stream);                                                                  /* PnP.py:1030-1074 */
/* argmax (+CRF marginals when from_crf) -> remap -> uint8 labels (concatenated, sum H*W) and, when
 * d_gt was given, hist[n_class*gt + pred] += 1 for 0 <= gt < n_class (PnP.py:1106-1146; the flat np.bincount index: a
 * pred >= n_class counts in the next row, an index >= n_class^2 is dropped). d_hist: n_class*n_class uint64. */
int pnp_remap_hist(pnp_engine* e, int32_t from_crf, uint8_t* d_labels, unsigned long long* d_hist, int32_t n_class,
                   void* stream);
/* merge -> threshold/upsample -> [blur] -> [crf] -> argmax/remap/hist.  mode: bit0 blur, bit1 crf. */
int pnp_postprocess(pnp_engine* e, const float* d_gradcam, int32_t T, float threshold, int32_t scale01, int32_t mode,
                    uint8_t* d_labels, unsigned long long* d_hist, int32_t n_class, void* stream);

/* Both post-processing branches of a batch -- 1-drop (PnP.py:348-403, with Scale_0_1) and N-drop (PnP.py:424-481) --
 * with "blur+crf" in one DenseCRF run: the two problems share the image's lattices, so they are iterated side by side
 * (two channel groups per row).  Results equal two pnp_postprocess(..., mode 3, ...) calls bit for bit.
 * scale01_mask: bit 0 = Scale_0_1 on the 1-drop maps, bit 1 = on the N-drop maps (PnP.py: 1; the COCO driver
 * PnP_OVSS_0514_updated_segmentation_coco.py:436,527 scales both: 3). */
int pnp_postprocess_pair(pnp_engine* e, const float* d_gradcam_1drop, const float* d_gradcam_ndrop, int32_t T, float threshold,
                         int32_t scale01_mask, uint8_t* d_labels_1drop, unsigned long long* d_hist_1drop, uint8_t* d_labels_ndrop,
                         unsigned long long* d_hist_ndrop, int32_t n_class, void* stream);

/* ---- stand-alone DenseCRF: replaces pydensecrf's DenseCRF2D as the reference's densecrf() drives it (PnP.py:1063-1073) ----
 * The mean-field of pnp_densecrf on unary energies the caller brings and with kernel widths the caller chooses, in a solver
 * that owns its workspace and needs no pnp_engine: setUnaryEnergy + addPairwiseGaussian(sxy = pos_xy, compat = pos_w) +
 * addPairwiseBilateral(sxy = bi_xy, srgb = bi_rgb, compat = bi_w) + inference(iters) for a batch of images of any sizes and
 * label counts.  Potts compatibility, isotropic widths, DIAG_KERNEL / NORMALIZE_SYMMETRIC (pydensecrf's defaults).
 * pnp_crf_create allocates every device byte the solver will use (what pnp_post_reserve allocates for the CRF stage):
 * at most 64 images per batch and 255 labels per image, PNP_ERR_ARG beyond (and nothing is allocated).  On a later failure
 * (out of memory) *out is still a handle: pnp_crf_last_error says why, pnp_crf_destroy frees it.
 * A solver is not thread-safe; distinct solvers are independent.  Null pointers, B < 1, K < 2, non-positive widths and
 * iters < 0 are refused before any HIP call. */
typedef struct pnp_crf pnp_crf;
int pnp_crf_create(int32_t device, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image, int32_t max_labels,
                   pnp_crf** out);
void pnp_crf_destroy(pnp_crf* c);
size_t pnp_crf_allocated_bytes(const pnp_crf* c);
const char* pnp_crf_last_error(const pnp_crf* c);         /* valid until the next call on c; "null solver" for NULL */
typedef struct pnp_crf_batch {
    int32_t B;
    const int32_t* H;            /* [B] host */
    const int32_t* W;            /* [B] host */
    const int32_t* K;            /* [B] host: labels of image b, 2..max_labels */
    const uint8_t* d_rgb;        /* device: concatenated (H, W, 3) uint8 images */
    const float* d_unary;        /* device: concatenated (K_b, H_b * W_b) channel-major blocks (pydensecrf's setUnaryEnergy layout) */
} pnp_crf_batch;
/* Lays the batch out, copies the unary energies into the solver (d_unary may be reused once the stream has passed this call)
 * and builds both permutohedral lattices and their normalisers for these widths; the Gaussian lattice is kept while the image
 * sizes and pos_xy stay the same.  Synchronises (lattice size + key-range flag, once per lattice built).  A batch beyond the
 * reserved bounds is PNP_ERR_ARG with the numbers in pnp_crf_last_error; so is a colour (or position) width so small that a
 * lattice coordinate leaves the packed key -- the message names bi_rgb and the limit.  After a failed call the solver holds no
 * batch: pnp_crf_infer returns PNP_ERR_STATE until a pnp_crf_set_batch succeeds. */
int pnp_crf_set_batch(pnp_crf* c, const pnp_crf_batch* batch, float pos_xy, float bi_xy, float bi_rgb, void* stream);
/* Q0 = softmax(-U), then `iters` mean-field updates with weights pos_w / bi_w (a weight of 0 drops that kernel's term
 * arithmetically; both lattices are filtered all the same).  d_q (may be NULL): the marginals as (K_b, H_b * W_b) blocks, laid
 * out like d_unary; d_labels (may be NULL): uint8 argmax over the labels -- first maximum, a NaN wins, as np.argmax --
 * concatenated H_b * W_b.  May be called repeatedly on one batch; allocates nothing and does not synchronise. */
int pnp_crf_infer(pnp_crf* c, int32_t iters, float pos_w, float bi_w, float* d_q, uint8_t* d_labels, void* stream);
/* ---- beyond the reference's own call: per-axis widths, label-compatibility matrices, stepwise inference, KL divergence ----
 * What pydensecrf users do besides (sxy = (sx, sy), srgb = (sr, sg, sb); compat as a vector or matrix; startInference /
 * stepInference / klDivergence).  Still one Gaussian and one bilateral term, DIAG_KERNEL, NORMALIZE_SYMMETRIC.
 *
 * pnp_crf_set_batch_aniso: pnp_crf_set_batch with one width per feature axis -- Gaussian features (x / pos_xy[0],
 * y / pos_xy[1]), bilateral (x / bi_xy[0], y / bi_xy[1], r / bi_rgb[0], g / bi_rgb[1], b / bi_rgb[2]).  Equal widths build the
 * lattices of pnp_crf_set_batch bit for bit.  The Gaussian lattice is kept while the sizes and BOTH its widths stay the same.
 * Synchronises as pnp_crf_set_batch does. */
int pnp_crf_set_batch_aniso(pnp_crf* c, const pnp_crf_batch* batch, const float pos_xy[2], const float bi_xy[2], const float bi_rgb[3],
                            void* stream);
/* Label compatibility of term 0 (Gaussian) or 1 (bilateral), as MESSAGE WEIGHTS, used as given: with msg_t[k] the term's
 * filtered, normalised marginal of label k at a pixel, the update is
 *     logit[l] = (-U[l] + sum_k Mg[l][k] msg_g[k]) + sum_k Mb[l][k] msg_b[k],   Q = softmax(logit)
 * each sum in one fp32 accumulator, k ascending, products and sums rounded separately.  PNP_CRF_COMPAT_SCALAR: M = w I with the
 * w of the call (pos_w / bi_w; Potts, the default; host_values and K are not read); _DIAGONAL: host_values[K], M = diag(v);
 * _MATRIX: host_values[K * K] row-major, M[l][k] = host_values[l * K + k].  M = w I gives the scalar kind's marginals bit for
 * bit.  The values are copied into the solver (synchronises the device) and hold until changed, across batches.  A vector or
 * matrix needs K labels in every image of the batch: otherwise pnp_crf_infer / _step / _kl return PNP_ERR_ARG, and the solver
 * stays usable.  While both terms are scalar the Potts kernel runs and nothing differs from before.
 * Sign and symmetry are the caller's: densecrf's PottsCompatibility(w) is M = w I here; its DiagonalCompatibility(v) and
 * MatrixCompatibility(m) are M = diag(-v) and M = -(m + m^T) / 2 as this project reads densecrf (shims/general/pydensecrf converts) --
 * pinned by nothing the reference holds (oracle/README.md). */
enum { PNP_CRF_COMPAT_SCALAR = 0, PNP_CRF_COMPAT_DIAGONAL = 1, PNP_CRF_COMPAT_MATRIX = 2 };
int pnp_crf_set_compat(pnp_crf* c, int32_t term, int32_t kind, const float* host_values, int32_t K);
/* Stepwise inference on the batch of the last set_batch.  pnp_crf_start: Q = softmax(-U).  pnp_crf_step: n >= 0 more mean-field
 * updates from the current Q (start + step(a) + step(b) leaves the Q of pnp_crf_infer(a + b), bit for bit).  pnp_crf_read: the
 * current marginals (d_q) and their argmax (d_labels), laid out as pnp_crf_infer's outputs; either may be NULL.
 * pnp_crf_infer leaves the stepwise state equal to its result.  PNP_ERR_STATE while no batch is set, and from step / read /
 * kl while neither start nor infer has run on this batch.  None of them allocates; start / step / read do not synchronise. */
int pnp_crf_start(pnp_crf* c, void* stream);
int pnp_crf_step(pnp_crf* c, int32_t n, float pos_w, float bi_w, void* stream);
int pnp_crf_read(pnp_crf* c, float* d_q, uint8_t* d_labels, void* stream);
/* KL divergence of the current Q, one value per image into h_out_per_image[B] (host):
 *     sum_il Q log(max(Q, 1e-20)) + sum_il Q U - sum_t sum_il Q[i][l] acc_t[i][l],   acc_t[l] = sum_k M_t[l][k] msg_t[k] at this Q
 * Costs one filter pass per term; Q is not changed.  Products in fp32, the sum in fp64 in a fixed order (per pixel; then runs
 * of 256 pixels in pixel order; then the runs of an image in order), so the value is deterministic and does not depend on the
 * launch grid.  Synchronises.  This is densecrf's klDivergence as this project reads it (up to the constant densecrf leaves
 * out as well); like the rest of the CRF it is pinned by nothing the reference holds (oracle/README.md). */
int pnp_crf_kl(pnp_crf* c, float pos_w, float bi_w, double* h_out_per_image, void* stream);
/* ---- any number of pairwise terms over features the caller brings (pydensecrf's addPairwiseEnergy) ----
 * T = 1 .. max_terms terms; term t has d_t = 1 .. max_dims float32 features per pixel, ALREADY DIVIDED by their kernel widths
 * and used as given, and a compatibility of its own (scalar weight, vector or matrix: message weights as pnp_crf_set_compat
 * documents them).  Per term: the permutohedral embedding of pnp_crf_set_batch on f[i] = F_t[i][pixel]; msg_t = norm_t *
 * lattice_t(norm_t * Q) with norm_t = 1 / sqrt(lattice_t(1) + 1e-20) (sequential splat in pixel order, d_t + 1 axis blurs,
 * slice with alpha = 1 / (1 + 2^-d_t)); acc_t[l] = sum_k M_t[l][k] msg_t[k] (one fp32 accumulator, k ascending; a scalar:
 * w_t * msg_t[l]).  Update: logit = ((-U + acc_0) + acc_1) + ... + acc_{T-1} in term order, Q = softmax(logit).  With T = 2,
 * F_0 = (x / sx, y / sy), F_1 = (x / sx, y / sy, r / sr, g / sg, b / sb) this is pnp_crf_infer's arithmetic bit for bit.
 * DIAG_KERNEL and NORMALIZE_SYMMETRIC only.
 *
 * pnp_crf_create_terms: pnp_crf_create for max_terms <= 8 terms of max_dims <= 6 feature axes.  D = 1 .. 6 and worst-case
 * sizing are the contract: every term gets a lattice for max_dims + 1 points per pixel (what a noisy feature can reach: 5.2 -
 * 5.5 at D = 6), and one pair of value buffers of that many rows per pixel serves all terms in turn;
 * pnp_crf_allocated_bytes reports the total, and a failed allocation leaves a handle whose pnp_crf_last_error says how many
 * bytes were wanted.  The solver serves pnp_crf_set_batch* / pnp_crf_infer as one of pnp_crf_create does.
 *
 * pnp_crf_set_batch_terms: batch->d_rgb is not read.  terms[t].d_features (device) holds the (dims, H_b * W_b) blocks of the
 * images back to back, as d_unary holds the (K_b, H_b * W_b) blocks; it is read during this call only.  Builds every lattice
 * and normaliser; synchronises once per lattice.  The lattice key holds min(16, 64 / dims) bits per coordinate (no image
 * bits): |coordinate| < 505 at dims = 6, < 2042 at dims = 5, < 32000 below.  A coordinate beyond it, or a feature that is not
 * finite, is PNP_ERR_ARG: the message names the term and the limit, and a wider kernel width is the remedy.  After a failed
 * call the solver holds no batch.
 *
 * pnp_crf_set_term_compat: pnp_crf_set_compat for term < max_terms of the feature path (pnp_crf_set_compat itself keeps to
 * the Gaussian / bilateral terms 0 and 1 of the two-term path; the two sets of compatibilities are separate).
 * pnp_crf_infer_terms / pnp_crf_step_terms: pnp_crf_infer / pnp_crf_step with weights[T] (host), the weight of every term left
 * scalar.  pnp_crf_start and pnp_crf_read serve both kinds of batch; start + step_terms(a) + step_terms(b) leaves the Q of
 * infer_terms(a + b) bit for bit.  The two-term calls on a terms batch and the terms calls on a two-term batch return
 * PNP_ERR_STATE; pnp_crf_kl on a terms batch returns PNP_ERR_ARG (not available).  Null pointers and counts out of range are
 * refused before any HIP call. */
enum { PNP_CRF_MAX_TERMS = 8, PNP_CRF_MAX_DIMS = 6 };
typedef struct pnp_crf_term {
    int32_t dims;                /* feature axes of the term, 1..max_dims */
    const float* d_features;     /* device: concatenated (dims, H_b * W_b) blocks */
} pnp_crf_term;
int pnp_crf_create_terms(int32_t device, int32_t max_batch, int64_t max_total_pixels, int32_t max_pixels_per_image, int32_t max_labels,
                         int32_t max_terms, int32_t max_dims, pnp_crf** out);
int pnp_crf_set_batch_terms(pnp_crf* c, const pnp_crf_batch* batch, int32_t n_terms, const pnp_crf_term* terms, void* stream);
int pnp_crf_set_term_compat(pnp_crf* c, int32_t term, int32_t kind, const float* host_values, int32_t K);
int pnp_crf_infer_terms(pnp_crf* c, int32_t iters, const float* weights, float* d_q, uint8_t* d_labels, void* stream);
int pnp_crf_step_terms(pnp_crf* c, int32_t n, const float* weights, void* stream);
/* Lattice points of one term over the whole batch, as the last successful set_batch built it: term < T of a terms batch; 0
 * (Gaussian) or 1 (bilateral) of a two-term batch.  -1 for a null solver, no batch, or no such term. */
int64_t pnp_crf_lattice_points(const pnp_crf* c, int32_t term);
/* ---- a term's lattice, stage by stage (for tests: what a lattice build left, and parts of one filter pass) ----
 * pnp_crf_lattice_view_get: the arrays of one term's lattice as the last successful set_batch left them -- device pointers into the
 * solver's workspace, valid until the next set_batch or pnp_crf_destroy, to be read only -- and their sizes.  term as
 * pnp_crf_lattice_points takes it.  Returns pointers and sizes: it allocates nothing, does not synchronise (set_batch did) and
 * writes no device memory.  Lattice ids are internal: points are numbered image by image (idbase) along a Z-order curve of
 * their first contributor pixel; every id below is global to the batch except those of nbr8, which are local to the image.
 * PNP_ERR_ARG: null solver or view, no such term; PNP_ERR_STATE: no batch is set. */
typedef struct pnp_crf_lattice_view {
    int32_t D1;                  /* d + 1: lattice points per pixel, and blur axes */
    int32_t images;              /* B */
    int64_t cap;                 /* stride, in points, of the axis tables n1 / n2 / nbr8 */
    int64_t points;              /* M = idbase[B] */
    int64_t entries;             /* (pixels of the batch) * D1 */
    const float* bary;           /* [entries] barycentric weight of (pixel, vertex) = pixel * D1 + vertex */
    const int32_t* offset;       /* [entries] lattice id of (pixel, vertex) */
    const uint32_t* vals;        /* [entries] contributor lists: (pixel, vertex) indices, point by point in id order */
    const void* ent;             /* [entries] the same lists as 16-byte records {uint32 pixel, float w, float nr, uint32 pad} */
    const int32_t* seg_lo;       /* [M] a point's contributors are vals[seg_lo .. seg_hi) */
    const int32_t* seg_hi;
    const int32_t* idbase;       /* [B + 1] first lattice id of every image */
    const int32_t* n1;           /* [D1][cap] blur neighbours along every axis, -1 = absent */
    const int32_t* n2;
    const void* nbr8;            /* [D1 / 2][cap] 32-byte records {ia, id, pa, pd, aa, ad, da, dd} (int32) of the two-axis blur */
    const float* norm;           /* [pixels of the batch] the term's normaliser */
} pnp_crf_lattice_view;
int pnp_crf_lattice_view_get(pnp_crf* c, int32_t term, pnp_crf_lattice_view* out);
/* pnp_crf_probe_filter: part of one filter pass of `term` on rows the caller brings, through the kernels and the dispatch of the
 * mean-field itself.  d_in: (K_b, H_b * W_b) float32 planes laid out as d_unary; they take the place of the marginals.  stage:
 *   PNP_CRF_PROBE_SPLAT    the splat alone
 *   PNP_CRF_PROBE_FORWARD  splat and the D1 blur axes as an update runs them (axes in pairs, a single last axis)
 *   PNP_CRF_PROBE_REVERSE  splat and the axes D1 - 1 .. 0 one by one, as the backward pass runs them
 *   PNP_CRF_PROBE_SLICE    the message of the forward result: norm * alpha * slice
 * d_out, SPLAT / FORWARD / REVERSE: the value rows of the lattice without their padding, K_b floats per lattice point in id
 * order, image after image: sum_b (idbase[b + 1] - idbase[b]) * K_b floats.  SLICE: planes laid out as d_in.  The solver's
 * marginals are overwritten and its stepwise state is dropped (pnp_crf_start begins anew).  A two-term solver allocates B
 * descriptors on its first probe of term 1 (counted in pnp_crf_allocated_bytes).  Errors as pnp_crf_lattice_view_get; a stage
 * out of range or a null pointer is PNP_ERR_ARG. */
enum { PNP_CRF_PROBE_SPLAT = 0, PNP_CRF_PROBE_FORWARD = 1, PNP_CRF_PROBE_REVERSE = 2, PNP_CRF_PROBE_SLICE = 3 };
int pnp_crf_probe_filter(pnp_crf* c, int32_t term, int32_t stage, const float* d_in, float* d_out, void* stream);
/* ---- gradients of the feature-term mean-field (reverse mode; densecrf's DenseCRF::gradient) ----
 * The mean-field of pnp_crf_infer_terms as a differentiable function of the unary energies and of the terms' compatibilities
 * (scalar weight, vector, matrix).  Features, lattices and normalisers are constants of the batch.  Term t's operator A_t =
 * alpha N S^T B_d .. B_0 S N (splat S, axis blurs B_j, normaliser N) is not symmetric for d >= 2; its adjoint runs the blur axes in
 * reverse order, and that is what the backward pass filters with.
 *
 * pnp_crf_reserve_grad: allocates the gradient workspace of a solver of pnp_crf_create_terms, once (further calls return
 * PNP_OK and allocate nothing; a call after one that ran out of memory allocates what is missing): four row arrays of the size
 * of Q (cotangent, dl, h, unary gradient), a buffer for the per-tile fp32 partials of the compatibility gradients -- a batch
 * with more tiles than it holds (thin images, 1-D signals) passes through it in spans, with the same bits -- and their fp64 sums.  Counted in pnp_crf_allocated_bytes; a solver that never calls it
 * allocates what it did before.  PNP_ERR_STATE on a solver of pnp_crf_create.
 *
 * pnp_crf_infer_terms_saved: pnp_crf_infer_terms -- the same kernels, launches and arithmetic, d_q and d_labels bit for bit --
 * which also copies the solver's pixel-major marginal rows into d_history after the start and after every update: iters + 1
 * blocks of sum_b Kp_b * H_b * W_b floats (Kp_b = K_b rounded up to a multiple of 4), caller-owned device memory.
 *
 * pnp_crf_backward_terms: from d_grad_q, the cotangent of the marginals laid out as d_q, the gradient of the unary energies
 * into d_grad_unary (laid out as d_unary) and, for every t < T with d_grad_compat[t] non-null (device memory; the array itself
 * is host memory of T pointers and may be NULL for none), the gradient of term t's compatibility: 1 float (scalar), K (vector)
 * or K * K (matrix, row-major [l][k]), float32 from fp64 sums.  It uses the batch and the compatibilities the solver holds and
 * `weights` for scalar terms, and d_history as pnp_crf_infer_terms_saved left it for the same iters: that these agree is the
 * caller's contract, nothing here can check it.  The message A_t Q_{i-1} is recomputed (one forward filter) only for terms whose
 * compatibility gradient is asked for.  No floating-point atomics: every sum runs in an order the batch fixes, two calls give
 * the same bits.  The solver's marginals and stepwise state stay as they were (pnp_crf_step_terms / pnp_crf_read go on as if
 * the call had not happened).  PNP_ERR_STATE: no terms batch is set, or pnp_crf_reserve_grad was not called.  PNP_ERR_ARG:
 * null pointers, iters < 0. */
int pnp_crf_reserve_grad(pnp_crf* c);
int pnp_crf_infer_terms_saved(pnp_crf* c, int32_t iters, const float* weights, float* d_history, float* d_q, uint8_t* d_labels,
                              void* stream);
int pnp_crf_backward_terms(pnp_crf* c, int32_t iters, const float* weights, const float* d_history, const float* d_grad_q,
                           float* d_grad_unary, float* const* d_grad_compat, void* stream);

/* ---- input side ("next" row: the tensors the reference's datasets hand to the model) -------
 * Dataset.py:434-443: transforms.Resize((S, S), BICUBIC) on the PIL image -> ToTensor -> Normalize(mean, std).
 * Pillow's 8-bit two-pass resampler (src/libImaging/Resample.c) in integer arithmetic, bit-exact: per axis and
 * output index o the host supplies (first tap, tap count) and 22-bit fixed-point taps (pnp_ovss.hip
 * .resample_table, the double-precision recipe of precompute_coeffs / normalize_coeffs_8bpc);
 * out = clip8((2^21 + sum taps * pixel) >> 22), horizontal pass first with a uint8 intermediate; then
 * (v / 255 - mean[c]) / std[c] in fp32.  Stateless; all pointers are device pointers except mean3 / std3. */
typedef struct pnp_pre_image {
    int64_t src_off;            /* byte offset of the image in d_rgb (H*W*3, row-major HWC uint8) */
    int64_t tmp_off;            /* byte offset of its H x S x 3 intermediate in d_tmp */
    int32_t H, W;
    int32_t kx_off, kx_size;    /* horizontal table at d_coef[kx_off]: S x (2 + kx_size) int32 = first, count, taps... */
    int32_t ky_off, ky_size;    /* vertical table, same layout */
} pnp_pre_image;
int pnp_preprocess_images(const uint8_t* d_rgb, const pnp_pre_image* d_desc, int32_t B, int32_t S, int32_t max_H,
                          const int32_t* d_coef, uint8_t* d_tmp, const float* mean3, const float* std3, float* d_out,
                          void* stream);

/* Dataset.py:349-445 / PnP.py:929-955 `Image.open(path).convert('RGB')` on device, for baseline (sequential Huffman, 8-bit,
 * grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0) JPEG files: Pillow = libjpeg(-turbo) defaults, restated bit-exactly (islow
 * integer IDCT, fancy chroma upsampling, fixed-point YCbCr -> RGB).  The host parses the markers (pnp_ovss/jpeg.py) and
 * hands over the entropy-coded bytes, the file's own DHT / DQT tables and these descriptors.  Entropy decode: one workgroup
 * per restart segment; the segment is cut into up to 1024 sub-sequences decoded by one thread each from a guessed decoder
 * state, then re-decoded from the predecessor's exit state until no entry state changes (Huffman streams self-synchronise;
 * the fixed point IS the sequential decode), block counts and DC differences are prefix-summed and a last pass writes the
 * coefficients.  Output: the images' RGB bytes (H*W*3, HWC) at rgb_off -- the buffer pnp_preprocess_images and
 * pnp_post_batch.d_rgb read.  Workspaces: d_clean (sum of clean_cap bytes: the un-stuffed streams), d_seg_bits (n_segments
 * ints).  *d_err is set to 1 on a corrupt or truncated stream.  Stateless. */
typedef struct pnp_jpeg_image {
    int64_t data_off;           /* offset of the entropy-coded segment in d_data, a multiple of 16 */
    int64_t coef_off[3];        /* int16 elements: quantised coefficient blocks [blocks_y][blocks_x][64] per component */
    int64_t plane_off[3];       /* bytes: component sample planes, row stride blocks_x * 8 */
    int64_t rgb_off;            /* bytes */
    int32_t data_len, H, W, ncomp, hmax, vmax, mcux, mcuy;
    int32_t h[3], v[3], tq[3], td[3], ta[3], bx[3], by[3];
    int32_t tab, pad[2];
} pnp_jpeg_image;
typedef struct pnp_jpeg_tables {
    uint8_t counts[4][16];      /* [DC0, DC1, AC0, AC1]: DHT code counts per length 1..16 ... */
    uint8_t vals[4][256];       /* ... and symbols, as in the file (the look-ahead tables are built on the device) */
    int32_t quant[4][64];       /* natural (row-major) order */
} pnp_jpeg_tables;
typedef struct pnp_jpeg_segment {
    int64_t byte_off;           /* first byte of the restart interval, relative to data_off */
    int64_t clean_off;          /* offset of its un-stuffed copy in d_clean, a multiple of 16 */
    int32_t image, mcu0, nmcu;
    int32_t raw_len;            /* entropy-coded bytes of the interval, markers excluded */
    int32_t clean_cap;          /* bytes reserved at clean_off, >= raw_len + 32 */
    int32_t sub_bits;           /* sub-sequence length in bits: a multiple of 32, >= 8 * raw_len / 1024 */
    int32_t scan;               /* pnp_jpeg_decode_scans only: index of the segment's scan in d_scans */
    int32_t pad;
} pnp_jpeg_segment;
int pnp_jpeg_decode(const uint8_t* d_data, const pnp_jpeg_image* d_images, const pnp_jpeg_tables* d_tables,
                    const pnp_jpeg_segment* d_segments, int32_t n_images, int32_t n_segments, uint8_t* d_clean, int32_t* d_seg_bits,
                    int16_t* d_coef, int64_t coef_elems, uint8_t* d_planes, uint8_t* d_rgb, int32_t max_blocks_per_image,
                    int32_t max_pixels_per_image, int32_t* d_err, void* stream);

/* The same decode for any mix of baseline and PROGRESSIVE (SOF2, Huffman, 8-bit, same colour spaces) files, scan by scan.
 * The host (pnp_ovss/jpeg.py pack_scans) records every scan of every file -- a baseline file is one scan of kind 0 -- and has
 * checked the progression (T.81 G.1.1.1.1: every coefficient of every component ends at Al = 0).  One restart interval of one
 * scan is one segment; `scan` names its pnp_jpeg_scan, mcu0 / nmcu count that scan's units: MCUs of the frame in an
 * interleaved scan, blocks of the component's own ceil(Xc / 8) x ceil(Yc / 8) grid (bw x bh) in a one-component scan.
 * d_segments holds the n_base_segments segments of baseline files first, then the progressive ones ordered by (scan ordinal,
 * kind): h_groups, a HOST array of n_groups x 4 int32 (first segment, segments, kind, ordinal) in that order, names the
 * contiguous ranges, one launch each, so every file's scans run in file order.  Order of work: zero the coefficients, un-stuff
 * all segments, baseline entropy decode, the groups, inverse DCT + colour over all images.  The four progressive kinds restate
 * T.81 G.1.2 (csrc/jpeg_prog.hip); the Huffman ones use the sub-sequence scheme above.  An image's `tab` entry holds its
 * quantisation tables (tq indexes it), a scan's `tab` entry the Huffman tables in force at its SOS.
 * Workspaces as pnp_jpeg_decode, plus d_hist: coef_elems / 64 uint64, one history mask per coefficient block (AC refinement).
 * d_rounds (device, n_segments ints, may be NULL): synchronisation rounds each progressive segment took.  h_group_ms (host,
 * n_groups floats, may be NULL): profiling -- every group's launch is timed between two events and the call synchronises.
 * *d_err is set to 1 on an undefined code, a size above 1 in a refinement symbol, an index past Se, an end-of-band run past
 * the scan's blocks or a stream that ends early.  Stateless; PNP_ERR_ARG for inconsistent arguments before any HIP call. */
typedef struct pnp_jpeg_scan {
    int32_t image;
    int32_t kind;               /* 0 sequential, 1 DC first, 2 DC refinement, 3 AC first, 4 AC refinement */
    int32_t ordinal;            /* position of the scan in its file */
    int32_t ncomp, comp[3];     /* the scan's components, indices into the frame, in frame order */
    int32_t td[3], ta[3];       /* per scan component: slot (0 / 1) of its DC / AC Huffman table in d_tables[tab] */
    int32_t ss, se, ah, al;     /* spectral selection and successive approximation of the SOS header */
    int32_t tab;
    int32_t bw, bh;             /* the grid the scan's units are counted on */
    int32_t nunits;             /* bw * bh */
    int32_t pad[3];
} pnp_jpeg_scan;
int pnp_jpeg_decode_scans(const uint8_t* d_data, const pnp_jpeg_image* d_images, const pnp_jpeg_tables* d_tables,
                          const pnp_jpeg_scan* d_scans, const pnp_jpeg_segment* d_segments, int32_t n_images, int32_t n_scans,
                          int32_t n_segments, int32_t n_base_segments, const int32_t* h_groups, int32_t n_groups, uint8_t* d_clean,
                          int32_t* d_seg_bits, int16_t* d_coef, int64_t coef_elems, uint64_t* d_hist, uint8_t* d_planes,
                          uint8_t* d_rgb, int32_t max_blocks_per_image, int32_t max_pixels_per_image, int32_t* d_rounds,
                          float* h_group_ms, int32_t* d_err, void* stream);

/* ---- output side: what the reference's Draw_Segmentation_map writes (PnP_OVSS_0514_updated_segmentation_coco.py:966-983) ----
 * Colour overlay of label maps on their images: skimage.color.label2rgb(kind="overlay", alpha, bg_label=0, image_alpha=1,
 * saturation=0) followed by matplotlib's float -> uint8 conversion, in double precision and in this order:
 *   g = (0.2125 R + 0.7154 G + 0.0721 B) / 255;  label 0: out_c = uint8(g * 255);
 *   label l > 0: out_c = uint8((palette[l][c] / 255 * alpha + g * (1 - alpha)) * 255)       (truncation).
 * d_labels: the concatenated uint8 label maps of B images (pnp_remap_hist / pnp_postprocess output), d_rgb / d_out: the
 * concatenated HWC uint8 images (pnp_post_batch.d_rgb), d_pix_off: int64[B + 1] pixel offsets of the images (only the total
 * d_pix_off[B] matters: the operation is per pixel), d_palette: uint8[256 * 3] indexed by label -- the colour of a class does
 * not depend on which other classes an image holds (the reference colours by rank among the labels present).
 * 0 <= alpha <= 1.  Stateless. */
int pnp_overlay_labels(const uint8_t* d_labels, const uint8_t* d_rgb, const int64_t* d_pix_off, int32_t B,
                       const uint8_t* d_palette, double alpha, uint8_t* d_out, void* stream);

/* Baseline JPEG encode of a batch of HWC uint8 RGB images of any sizes: the entropy-coded scan (0xFF00-stuffed, last byte
 * padded with 1-bits, no markers) that libjpeg writes with its defaults -- YCbCr 4:2:0, islow integer DCT, the T.81 Annex K
 * Huffman tables, no restart markers -- so that markers + scan + EOI (pnp_ovss/jpeg.py) equal Pillow's
 * Image.save(buf, "JPEG", quality=q) byte for byte.  h_images: HOST array of n_images descriptors; h_quant: HOST uint16[2][64],
 * the luma and chroma quantisation tables in natural order, values 1..255.  Image i's scan goes to d_out + out_off and its
 * length to d_out_len[i]; an image whose scan would exceed out_cap gets d_out_len[i] = -1, sets *d_err = 1 and has nothing
 * written, the other images are unaffected (*d_err is 0 otherwise).  d_ws: workspace of at least *ws_need bytes, 256-byte
 * aligned; a call with d_ws = NULL only computes *ws_need for these descriptors.  At most 2^31 / 1664 blocks of 8 x 8 per call
 * (215 000 MCUs: 280 images of 500 x 375), PNP_ERR_ARG beyond.  Stateless; nothing is read back to the host. */
typedef struct pnp_jpeg_enc_image {
    int64_t rgb_off;            /* byte offset of the image in d_rgb (H*W*3, row-major HWC uint8) */
    int64_t out_off;            /* byte offset of its scan in d_out */
    int32_t H, W;               /* 1..65535 */
    int32_t out_cap;            /* bytes reserved at out_off */
    int32_t pad;
} pnp_jpeg_enc_image;
int pnp_jpeg_encode(const uint8_t* d_rgb, const pnp_jpeg_enc_image* h_images, int32_t n_images, const uint16_t* h_quant,
                    uint8_t* d_out, int32_t* d_out_len, int32_t* d_err, void* d_ws, int64_t ws_bytes, int64_t* ws_need,
                    void* stream);

/* Label maps as 8-bit PNG files: the zlib stream of the IDAT chunk for a batch of uint8 label maps of any sizes, concatenated
 * in d_labels as pnp_remap_hist leaves them.  The host adds the chunk framing and its CRC-32 (pnp_ovss/png.py).  The bytes are
 * fixed by the format, not by a library: header 78 01; one deflate block with the fixed Huffman code (BFINAL = 1, BTYPE = 01);
 * end-of-block; zero bits to a whole byte; Adler-32 of the filtered stream, big-endian.  Per row the filter is Up (2) when the
 * Up-filtered row has fewer changes between neighbouring bytes than the raw row, None (0) otherwise; the W + 1 bytes of a row,
 * filter byte included, are cut into maximal runs of equal bytes, and a run of byte b and length r is: literal b, then
 * (r - 1) / 258 matches of length 258 at distance 1, then for t = (r - 1) % 258 one match of length t when t >= 3, t literals
 * otherwise (csrc/png_enc.hip; tests/_png_refs.py restates it).  h_images: HOST array of n_images descriptors.  Image i's
 * stream, zlib header and Adler-32 included, goes to d_out + out_off and its length to d_out_len[i]; an image whose stream
 * would exceed out_cap gets d_out_len[i] = -1, sets *d_err = 1 and has nothing written, the other images are unaffected
 * (*d_err is 0 otherwise).  No stream exceeds 2 + ceil((10 + 9 H (W + 1)) / 8) + 4 bytes.  d_ws: workspace of at least
 * *ws_need bytes, 256-byte aligned; a call with d_ws = NULL only computes *ws_need for these descriptors.  At most 2^31 / 9
 * bytes of filtered stream (the sum of H (W + 1)) per call, PNP_ERR_ARG beyond: bit offsets are int32.  The argument checks
 * run before any device is touched.  Stateless; nothing is read back to the host. */
typedef struct pnp_png_image {
    int64_t labels_off;         /* byte offset of the label map in d_labels (H*W, row-major uint8) */
    int64_t out_off;            /* byte offset of its stream in d_out */
    int32_t H, W;               /* 1..65535 */
    int32_t out_cap;            /* bytes reserved at out_off, >= 0 */
    int32_t pad;
} pnp_png_image;
int pnp_png_encode(const uint8_t* d_labels, const pnp_png_image* h_images, int32_t n_images, uint8_t* d_out, int32_t* d_out_len,
                   int32_t* d_err, void* d_ws, int64_t ws_bytes, int64_t* ws_need, void* stream);

/* ---- introspection (tests / profiling) --------------------------------------------------- */
/* Named internal device buffers: "image_embeds" (fp32 B*N*D), "text_hidden" (fp32 B*L*H: last_hidden_state of the most recent
 * text pass, multimodal or text-only), "maps" (fp32 post-process maps), "crf_q", "P", "dP", "crf_M" (int32 [2][B+1] lattice id
 * bases), ... */
int pnp_get_buffer(pnp_engine* e, const char* name, void** d_ptr, size_t* bytes);
/* Live kernel timing for bench.py's roofline line: while enabled, every launch of the dominant
 * kernel family (the dense NT GEMMs with M = B*N rows: gemm_nt_x3_kernel<EPI> in the benchmarked split-bf16 mode
 * (csrc/gemm_x3.hip; three bf16 MFMAs per product, so the MFMA work issued is 3x the FLOPs reported here),
 * gemm_nt_wide_kernel<EPI> in the bf16 throughput mode, gemm_nt_big_kernel<float> in the exact-fp32 mode) is
 * bracketed by hipEvents on the launch stream.  pnp_profile_read
 * synchronises those events and returns launches, summed algorithmic FLOPs (2*M*N*K) and summed
 * kernel milliseconds since the last enable.  Off by default (no events on the hot path).  on = 1 brackets every launch,
 * on = n > 1 every n-th launch of the family (an event pair costs ~2.5 us of stream serialisation; sums cover the bracketed
 * launches only). */
int pnp_profile_enable(pnp_engine* e, int32_t on);
int pnp_profile_read(pnp_engine* e, int64_t* launches, double* flops, double* ms);
/* Same for a pipeline stage: 0 = the dense GEMMs (as pnp_profile_read); 1 = the DenseCRF mean-field iterations
 * (PnP.py:1066-1072: splat / lattice blur / slice + update kernels of one batch, bracketed as a whole) with `work` =
 * SURVEY.md 8d's algorithmic bytes and nothing else: per mean-field iteration (2 x 9 + 2) x K x H x W x 4 (splat + slice over
 * the 3 + 6 simplex vertices of a pixel, Q read + written), summed over the iterations of the bracketed batches; 2 = the same
 * brackets (same launches, same ms) with `work` = the lattice term that 8d leaves out: 2 x (2 x M_gauss + 3 x M_bilateral) x K x 4
 * per iteration (the value arrays of the M_* lattice points read and written once per two-axis blur pass). */
int pnp_profile_read_stage(pnp_engine* e, int32_t stage, int64_t* launches, double* work, double* ms);
/* Process-wide tuning switches (diagnostics and A/B measurements; the defaults are what is benchmarked).
 *   "streamk": the stream-K tail of the persistent split-bf16 GEMM (the ViT Linears of B/vit.py:45-51, 93-117 at M = B * N rows):
 *              0 = whole tiles only, 1 (default) = the last partial round of tiles is cut along K over all CUs when the cost
 *              model says it pays, 2 = whenever a launch has a partial last round.  Results are deterministic in every
 *              mode (fixed-order fix-up, no atomics) and differ between modes only by fp32 summation order.  Launches on a
 *              stream that is being captured into a hipGraph always take whole tiles (the tail's one-launch-at-a-time event
 *              chain reaches across streams).  That chain -- at most one launch with a tail in flight per device, whatever the
 *              streams, host threads and epilogues -- holds within one process: several processes on one device are outside it.
 *   "text_rows": workgroups per (head, image) of the text self-attention launches for captions of 65..192 tokens (B/med.py:
 *              229-283 self-attention forward and its backward): 0 (default) = chosen per launch from B * heads, L and the CU
 *              count, 1..4 = that many wherever the choice is made.  The split decides which workgroup computes a row, not one
 *              operation of its arithmetic: results are bit-identical for every value.  In the fp32 backward 1 selects the
 *              one-launch form and 2..4 the two-launch form (query-row phase, then key-row phase).
 *   "gemm_stamps": 0 (default) | 1 = every launch of the generic, wide-tile and split-bf16 wide GEMM kernels records
 *              per-workgroup clock stamps for pnp_dbg_gemm_stamps.  There is one library build and it reads no environment
 *              variable: this switch is the only way to turn the stamps on, and they time the kernels every caller runs.
 *              The stamp buffer (8192 rows, 512 KB of device memory) is allocated by the first enable, on the device current at
 *              that moment, and kept; PNP_ERR_HIP if that allocation fails.  Launches on any other device, and launches of
 *              more than 8192 workgroups (the generic kernels run one per tile), record nothing and leave the buffer alone.
 *              Results are bit-identical with stamps on and off. */
int pnp_set_tuning(const char* key, int32_t value);
/* Launches that used the engine's (e = NULL: the op-level entry points') stream-K workspace, and the give-up word of its
 * bounded spins (0 = no owner ever gave up waiting for a partial tile; anything else is a bug report).  Synchronises. */
int pnp_streamk_status(pnp_engine* e, int64_t* launches, uint32_t* gave_up);
/* Stand-alone operator entry points used by the parity tests (device pointers, see csrc/). */
int pnp_op_gemm(int32_t bf16, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo, int32_t gelu,
                void* stream);
/* Same with the compute-type (bf16 / fp32) output and epilogue mode (0 linear, 1 GELU) exposed. */
int pnp_op_gemm_ex(int32_t bf16, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                   const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo, void* d_out_t,
                   int32_t ldo_t, int32_t mode, void* stream);
/* The transposed K / V projection form (B/vit.py:93-117 value, B/med.py:201-228 key/value with the image tokens
 * as output columns): out[m, (n / col_div) * col_pad + n % col_div] = A[m,:] . B[n,:] + bias_rows[m], output in
 * the compute type; col_div = 0 keeps n. */
int pnp_op_gemm_tokcols(int32_t bf16, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                        int32_t K, const float* d_bias_rows, void* d_out_t, int32_t ldo_t, int32_t col_div,
                        int32_t col_pad, void* stream);
/* Every field of a non-split launch (fp32 or bf16 operands) that the entry points above hide:
 *   out[row(m), col(n)] = act(A[m,:] . B[n,:] + bias) (+ resid), written to d_out_f32 and / or d_out_t (compute type), at
 *   least one of them;  mode 0 linear | 1 GELU (pre-activation stashed to d_aux[row(m), n] when given) | 2 multiply by
 *   GELU'(d_aux[row(m), n]) (d_aux required);  bias[n], or bias[m] with bias_on_rows;
 *   row_div > 0: row(m) = (m / row_div) * (row_div + 1) + 1 + m % row_div and resid = pos_embed [row_div + 1, ldr], read at
 *   row 1 + m % row_div (the patch-embed form, B/vit.py:274-283: token row 0 of every image is not written);
 *   col_div > 0: col(n) = (n / col_div) * col_pad + n % col_div (col_pad >= col_div), as pnp_op_gemm_tokcols.
 * Null operands, no output, non-positive sizes, lda / ldb < K, mode outside 0..2, mode 2 without d_aux, negative row_div /
 * col_div and col_pad < col_div return PNP_ERR_ARG before any HIP call.
 * Every non-split GEMM entry point (this one, pnp_op_gemm, pnp_op_gemm_ex, pnp_op_gemm_tokcols) returns PNP_ERR_ARG for
 * N % 4 != 0 together with a per-column bias, a residual or d_aux: the kernels read those four columns at a time, and the
 * last group would reach past column N.  N % 4 != 0 with bias_on_rows (or no bias) and no residual / d_aux is accepted. */
int pnp_op_gemm_args(int32_t bf16, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N, int32_t K,
                     const float* d_bias, int32_t bias_on_rows, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo,
                     void* d_out_t, int32_t ldo_t, int32_t mode, float* d_aux, int32_t ld_aux, int32_t row_div, int32_t col_div,
                     int32_t col_pad, void* stream);
/* Split-bf16 ("bf16x3") form of the Linear (compute mode 2): operands are bf16 pairs x = hi + lo (pnp_op_split),
 * out = A.B^T accumulated as A_hi.B_hi + A_hi.B_lo + A_lo.B_hi in fp32, then one of the fp32-facing epilogues:
 *   d_out_f32, no col_div / bias_on_rows : + bias[n] (+ resid)            -> fp32 [M, ldo]
 *   d_out_f32, bias_on_rows / col_div    : + bias[m], token-column remap  -> fp32 [M, ldo]   (as pnp_op_gemm_tokcols)
 *   gelu, d_out_hi + d_out_lo            : + bias[n], erf GELU            -> split bf16 pair [M, ldo_t]
 * The first and third need N % 4 == 0; the token-column form with an even col_div (or col_div = 0) needs an even N (token
 * pairs are stored together): PNP_ERR_ARG otherwise.  pnp_op_gemm_tokcols has no such limit. */
int pnp_op_split(const float* d_in, void* d_hi, void* d_lo, int64_t n, void* stream);
int pnp_op_gemm_x3(const void* d_A_hi, const void* d_A_lo, int32_t lda, const void* d_B_hi, const void* d_B_lo, int32_t ldb,
                   int32_t M, int32_t N, int32_t K, const float* d_bias, int32_t bias_on_rows, const float* d_resid, int32_t ldr,
                   float* d_out_f32, int32_t ldo, void* d_out_hi, void* d_out_lo, int32_t ldo_t, int32_t gelu, int32_t col_div,
                   int32_t col_pad, void* stream);
/* Text-side form of the split-bf16 Linear (B/med.py:201-228 query / key / value, :321-325 and :393-411 dense layers at
 * M = B*L rows, and their backward): A is fp32 [M, lda] and is split into (hi, lo) bf16 by the kernel, the weight is a
 * (hi, lo) bf16 pair; out[m, n] = act(A[m,:] . B[n,:] + bias[n]) (+ resid[m, n]) in fp32.
 *   mode 0 linear | 1 erf GELU (pre-activation stashed to d_aux when given) | 2 multiply by GELU'(d_aux[m, n]). */
int pnp_op_gemm_x3a(const float* d_A, int32_t lda, const void* d_B_hi, const void* d_B_lo, int32_t ldb, int32_t M, int32_t N,
                    int32_t K, const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo, int32_t mode,
                    float* d_aux, int32_t ld_aux, void* stream);
/* What the GEMM entry points above would launch for one problem: the library's own dispatch, computed on the host from the
 * launch's scalars.  Touches no device and takes no device pointer.
 *   form    : PNP_GEMM_FORM_* -- pnp_op_gemm* with bf16 = 0 / 1, pnp_op_gemm_x3, pnp_op_gemm_x3a
 *   has     : PNP_GEMM_HAS_* bits, the operands and outputs that are present
 *   n_cu    : compute units of the device; streamk_mode as pnp_set_tuning("streamk"); sk_wgs: workgroups the stream-K
 *             workspace was sized for (0 = none; the op-level entry points use n_cu)
 * plan->status is PNP_OK or the PNP_ERR_ARG the launch would return (also the return value); the other fields then are 0. */
enum { PNP_GEMM_FORM_F32 = 0, PNP_GEMM_FORM_BF16 = 1, PNP_GEMM_FORM_X3 = 2, PNP_GEMM_FORM_X3A = 3 };
enum { PNP_GEMM_HAS_BIAS = 1, PNP_GEMM_HAS_BIAS_ON_ROWS = 2, PNP_GEMM_HAS_RESID = 4, PNP_GEMM_HAS_OUT_F32 = 8, PNP_GEMM_HAS_OUT_T = 16,
       PNP_GEMM_HAS_OUT_LO = 32, PNP_GEMM_HAS_AUX = 64 };
enum { PNP_GEMM_G64 = 0, PNP_GEMM_G128 = 1, PNP_GEMM_G256 = 2, PNP_GEMM_WIDE = 3, PNP_GEMM_X3_WIDE = 4, PNP_GEMM_SMALL_X3 = 5 };
typedef struct pnp_gemm_plan {
    int32_t status;
    int32_t family;        /* PNP_GEMM_G64 .. PNP_GEMM_SMALL_X3: generic 64 / 128 / 256 tiles, wide bf16, wide split-bf16, text-side split */
    int32_t variant;       /* wide families: the compile-time epilogue (0 +bias -> bf16 | 1 +bias GELU -> bf16 | 2 +bias +resid -> fp32 |
                            * 3 token columns -> bf16 | 4 +bias -> fp32 | 5 token columns -> fp32 | 6 +bias GELU -> pair | 7 +bias -> pair);
                            * PNP_GEMM_SMALL_X3: 0 = 32-deep slabs, three-slot ring | 1 = 64-deep slabs | 2 = 32-deep slabs; else 0 */
    int32_t dtype_bf16;    /* effective operand type of the kernel (1 for the wide split form whatever was asked) */
    int32_t n_pad;         /* N rounded up to the family's column tile */
    int32_t grid, block, smem;     /* workgroups, threads per workgroup, bytes of dynamic LDS */
    int32_t keeps_stamps;  /* the launch records clock stamps while "gemm_stamps" is on (at most 8192 workgroups) */
    int32_t profiled;      /* the launch belongs to the families pnp_profile_enable brackets */
    int32_t sk_full, sk_upw;       /* stream-K: tiles walked whole, slab pairs per workgroup in the split tail (0, 0 = whole tiles only).
                                    * A stream that is being captured runs the plan of streamk_mode 0 instead */
} pnp_gemm_plan;
int pnp_op_gemm_plan(int32_t form, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t mode, int32_t has,
                     int32_t row_div, int32_t col_div, int32_t col_pad, int32_t n_cu, int32_t streamk_mode, int32_t sk_wgs,
                     pnp_gemm_plan* plan);
/* ViT self-attention of one block (B/vit.py:93-117): ctx = softmax(q k^T * scale) v per (image, head), head_dim 64.
 * d_qk [B*N, ld_qk]: q of head h at column h*64, k at column D + h*64; d_ctx [B*N, D].
 * fp32 mode: d_vt [D, ld_vt] = V^T, row h*64+d, column b*n_pad + token (n_pad a multiple of 64, pad columns zero).
 * bf16 mode: d_vt [B*N, ld_vt] = V in the natural layout, head h at column h*64 (e.g. the v third of fused q|k|v
 * rows); it is transposed by the kernel's LDS reads and n_pad is not used. */
int pnp_op_vit_attention(int32_t bf16, const void* d_qk, int32_t ld_qk, int32_t D, const void* d_vt, int32_t ld_vt,
                         int32_t n_pad, void* d_ctx, int32_t B, int32_t heads, int32_t N, float scale, void* stream);
/* The same attention in split-bf16 form (compute mode 2): d_qkv_hi / d_qkv_lo [B*N, ld_qkv] hold q | k | v of every head as
 * bf16 pairs (q of head h at column h*64, k at D + h*64, v at 2D + h*64); the context leaves as a pair [B*N, D]. */
int pnp_op_vit_attention_x3(const void* d_qkv_hi, const void* d_qkv_lo, int32_t ld_qkv, int32_t D, void* d_ctx_hi, void* d_ctx_lo,
                            int32_t B, int32_t heads, int32_t N, float scale, void* stream);
int pnp_op_layernorm(const float* d_x, const float* d_w, const float* d_b, float eps, int32_t rows, int32_t D,
                     float* d_y, void* stream);
/* Cross-attention over the image tokens as one operator (B/med.py:229-283 forward, its autograd backward):
 *   mode 0: probs = softmax(x . K^T / 8) -> d_probs ; out = probs . V          (d_nat = K rows, d_tr = V^T)
 *   mode 1: dP = dctx . V^T ; dS = probs (dP - rowsum(dP probs)) ; out = dS . K / 8   (d_nat = V rows, d_tr = K^T,
 *           d_probs read)
 *   mode 2: d_probs = dctx . V^T                                               (d_nat = V rows)
 * d_nat [B*N, ld_nat] token-major; d_tr [heads*64, ld_tr] with element (h*64+d, b*n_pad + n); x / out [B*L, ld]
 * in the compute type (bf16 or f32); d_probs fp32 [B, heads, L, n_stride]. head_dim is 64. */
int pnp_op_xattn(int32_t bf16, int32_t mode, const void* d_nat, int32_t ld_nat, const void* d_tr, int32_t ld_tr,
                 int32_t n_pad, const void* d_x, int32_t ldx, void* d_out, int32_t ldo, float* d_probs, int32_t n_stride,
                 int32_t B, int32_t L, int32_t N, int32_t heads, void* stream);
/* Diagnostics.  While pnp_set_tuning("gemm_stamps", 1) holds, every workgroup of a generic, wide-tile or split-bf16 wide
 * GEMM launch writes one row of 8 words: the shader clock (slots 0-3) and the 100 MHz wall clock (slots 4-7) at kernel
 * start (0), at two points in between that depend on the kernel (1, 2: see the stamp() calls in csrc/gemm.hip and
 * csrc/gemm_x3.hip) and after the workgroup's last store has drained (3).  Every launch writes into the same buffer, so
 * the rows describe the LAST stamped launch (rows past its grid keep what earlier launches left), and they are meaningful
 * only with one stream launching GEMMs at a time.  A launch of more than 8192 workgroups, or on another device than the
 * buffer's, writes no row.  This synchronises the device and copies the first max_blocks rows (at
 * most 8192) to host_out.  PNP_ERR_STATE until stamps have been enabled once in this process. */
int pnp_dbg_gemm_stamps(uint64_t* host_out, int32_t max_blocks);
int pnp_op_cast(int32_t to_bf16, const float* d_in, void* d_out, int64_t n, void* stream);
/* The device-wide primitives of the DenseCRF lattice build as operators (the reference reaches them through pydensecrf's
 * hash table, PnP_OVSS_0514_updated_segmentation.py:1066-1070: here the lattice is built by a STABLE radix sort of the
 * (pixel, vertex) keys and prefix sums, csrc/sort.hip).  pnp_op_sort_pairs sorts n (u64 key, u32 value) pairs by the key
 * bits [begin_bit, end_bit) into d_keys_out / d_vals_out, equal keys keeping their input order; the input arrays are
 * overwritten.  h_seg_off (HOST array of n_seg + 1 ascending item offsets from 0 to n, n_seg <= 64; NULL = one segment):
 * the items of a segment are sorted among themselves and stay in its range (the images of a batch).
 * pnp_op_scan_i32: d_out[i] = sum of d_in[0..i] (inclusive) or d_in[0..i-1] (exclusive); in place allowed.
 * Both operator forms allocate their scratch per call and synchronise the stream before they free it: they hold the host
 * until the stream has drained (the lattice build itself runs the same kernels in the solver's workspace and does not). */
int pnp_op_sort_pairs(uint64_t* d_keys_in, uint64_t* d_keys_out, uint32_t* d_vals_in, uint32_t* d_vals_out, int64_t n,
                      int32_t begin_bit, int32_t end_bit, const size_t* h_seg_off, int32_t n_seg, void* stream);
int pnp_op_scan_i32(const int32_t* d_in, int32_t* d_out, int64_t n, int32_t inclusive, void* stream);
/* The text-side kernels as operators (head_dim 64: H = 64 * heads; compute type T = bf16 or fp32 by the first argument).
 * Non-positive sizes and missing mandatory pointers return PNP_ERR_ARG before any HIP call; nothing is allocated or synchronised.
 * BertSelfAttention without cross-attention (B/med.py:229-283): d_qkv [B*L, 3H] T (q | k | v), d_mask (B, ld_mask) int64 with
 * 1 = attend, added as (1 - mask) * -10000 (B/med.py:851); d_ctx [B*L, H] T; d_probs fp32 [B, heads, L, L] or NULL.  L <= 512.
 * For L > 192 the probabilities pass through global memory: d_probs, else d_scratch (same shape; may be NULL otherwise).
 * A masked key of an image with a live key gets probability exactly 0; an image whose mask is all zeros gets the softmax of
 * its scores shifted by -10000 (fp32: only 2^-10 of a score survives the shift), never NaN. */
int pnp_op_text_self_attn(int32_t bf16, const void* d_qkv, const int64_t* d_mask, int32_t ld_mask, void* d_ctx, float* d_probs,
                          float* d_scratch, int32_t B, int32_t L, int32_t H, void* stream);
/* Its backward: d_dctx fp32 [B*L, H], d_probs as stashed by the forward, d_ds_scratch fp32 [B, heads, L, L] (receives dS =
 * P (dP - rowsum(dP P))), d_dqkv [B*L, 3H] T = dq | dk | dv. */
int pnp_op_text_self_attn_bwd(int32_t bf16, const void* d_qkv, const float* d_dctx, const float* d_probs, float* d_ds_scratch,
                              void* d_dqkv, int32_t B, int32_t L, int32_t H, void* stream);
/* LayerNorm with every output of the kernel, each optional: d_y fp32, d_yt T, d_yt_lo bf16 (= bf16(y - yt), bf16 != 0 and d_yt
 * required: the split-bf16 pair), d_xhat fp32 [rows, D], d_rstd fp32 [rows].  D <= 1024, D % 4 == 0. */
int pnp_op_layernorm_ex(int32_t bf16, const float* d_x, const float* d_w, const float* d_b, float eps, int32_t rows, int32_t D,
                        float* d_y, void* d_yt, void* d_yt_lo, float* d_xhat, float* d_rstd, void* stream);
/* dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy * w; d_dx fp32 and / or d_dxt T. */
int pnp_op_layernorm_bwd(int32_t bf16, const float* d_dy, const float* d_w, const float* d_xhat, const float* d_rstd, int32_t rows,
                         int32_t D, float* d_dx, void* d_dxt, void* stream);
/* BertEmbeddings before its LayerNorm (B/med.py:88-123): d_out[b, l, :] = d_word[id] + d_pos[l], id = d_ids[b, l] (d_ids (B,
 * ld_ids) int64, the first L columns are read), clamped to [0, vocab - 1]; enc_id >= 0 replaces the id of column 0
 * (B/blip_image_text_matching.py:238), enc_id < 0 keeps it.  H % 4 == 0, enc_id < vocab, ld_ids >= L. */
int pnp_op_text_embed(const int64_t* d_ids, int32_t ld_ids, const float* d_word, const float* d_pos, float* d_out, int32_t B,
                      int32_t L, int32_t H, int32_t enc_id, int32_t vocab, void* stream);
/* itm_head on token 0 (B/blip_image_text_matching.py:248): d_logits[b, c] = d_hlast[b, 0, :] . d_w[c, :] + d_bias[c], c < 2;
 * and the seed of the backward of sum_b logits[b, 1]: d_dh[b, l, :] = d_w[1, :] at l = 0, else 0. */
int pnp_op_itm_head(const float* d_hlast, const float* d_w, const float* d_bias, float* d_logits, int32_t B, int32_t L, int32_t H,
                    void* stream);
int pnp_op_itm_grad_seed(const float* d_w, float* d_dh, int32_t B, int32_t L, int32_t H, void* stream);
/* The ViT input kernels (B/vit.py:274-283).  pnp_op_patchify: d_img (B, 3, S, S) fp32, S = 16 P -> d_out [B*P*P, 768] T, column
 * c * 256 + i * 16 + j = pixel (c, 16 py + i, 16 px + j); patches flagged in d_dropped ((B, P*P) uint8, may be NULL) are zeros.
 * pnp_op_cls_rows: d_x[b, 0, :] = d_cls + d_pos[0, :] for d_x (B, N, D) fp32; the other rows are not touched. */
int pnp_op_patchify(int32_t bf16, const float* d_img, const uint8_t* d_dropped, void* d_out, int32_t B, int32_t S, int32_t P,
                    void* stream);
int pnp_op_cls_rows(const float* d_cls, const float* d_pos, float* d_x, int32_t B, int32_t N, int32_t D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNP_HIP_H */
