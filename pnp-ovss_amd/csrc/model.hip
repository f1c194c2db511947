// The model sequence of the engine (include/pnp_hip.h): ViT, cross K / V, text stack, ITC projection, analytic backward, GradCAM
// gather and the drop loop, each a list of launches of this directory's kernels on the caller's stream (the engine's state and
// the Linear helpers are engine.h; lifetime and weights are engine.hip).  Host logic, but for three small layout kernels
// (feat_to_tok_kernel, tok_to_feat_kernel, embed_reuse_kernel).  No allocation / sync inside these calls.
#include <cmath>

#include "engine.h"

using namespace pnp;

namespace {

// The two extra layouts the analytic backward reads (V token-major for text layers >= stash_layer, K^T feature-major for
// layers > stash_layer) as 32 x 32 LDS transposes of what the forward's two cross K / V GEMMs have just written, instead of
// two more GEMMs over the same products (split-bf16 mode: 0.56 ms of GEMM per forward against 0.18 ms of copies; the copies
// are also bit-identical to the forward's values, which two GEMMs with swapped operand roles are not).
//   feat_to_tok: src [R features, ld_src] with token column b * n_pad + t  ->  dst [(b * N + t), R]
__global__ void feat_to_tok_kernel(const float* __restrict__ src, int ld_src, int n_pad, float* __restrict__ dst, int R, int N) {
    __shared__ float t[32][33];
    const int b = blockIdx.z, r0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, tok = t0 + threadIdx.x;
        t[i][threadIdx.x] = (r < R && tok < N) ? src[(size_t)r * ld_src + (size_t)b * n_pad + tok] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int tok = t0 + i, r = r0 + threadIdx.x;
        if (r < R && tok < N) dst[((size_t)b * N + tok) * R + r] = t[threadIdx.x][i];
    }
}
//   tok_to_feat: src [(b * N + t), ld_src] columns c0 .. c0 + R  ->  dst [R features, ld_dst] at token column b * n_pad + t
__global__ void tok_to_feat_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst, int n_pad, int R, int N) {
    __shared__ float t[32][33];
    const int b = blockIdx.z, r0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int tok = t0 + i, r = r0 + threadIdx.x;
        t[i][threadIdx.x] = (r < R && tok < N) ? src[((size_t)b * N + tok) * ld_src + r] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = r0 + i, tok = t0 + threadIdx.x;
        if (r < R && tok < N) dst[(size_t)r * ld_dst + (size_t)b * n_pad + tok] = t[threadIdx.x][i];
    }
}

// Patch embeddings of a later drop iteration: the images are the ones of iteration 0 with more 16 x 16 blocks zeroed
// (PnP.py:597-603), so a token's embedding is either what iteration 0 computed or, for a dropped patch, bias + pos exactly as the
// GEMM epilogue forms it from a zero accumulator ((0 + bias[n]) + pos[t][n]); the cls row never changes.  One pass over x instead of
// patchify + the patch GEMM.
__global__ void embed_reuse_kernel(const float* __restrict__ x0, const uint8_t* __restrict__ dropped, const float* __restrict__ bias,
                                   const float* __restrict__ pos, float* __restrict__ x, int rows, int N, int D4) {
    const size_t total = (size_t)rows * D4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / D4), c = (int)(i - (size_t)m * D4);
        const int b = m / N, t = m - b * N;
        f32x4 v;
        if (t > 0 && dropped[(size_t)b * (N - 1) + (t - 1)]) {
            const f32x4 bv = reinterpret_cast<const f32x4*>(bias)[c];
            const f32x4 pv = reinterpret_cast<const f32x4*>(pos)[(size_t)t * D4 + c];
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = __fadd_rn(__fadd_rn(0.0f, bv[e]), pv[e]);
        } else {
            v = reinterpret_cast<const f32x4*>(x0)[i];
        }
        reinterpret_cast<f32x4*>(x)[i] = v;
    }
}

// Where a forward's token embeddings and text prefix come from:
//   fresh: compute the token embeddings (the operator form) | keep: compute them and keep a copy (drop iteration 0) | reuse: the
//   images are those of the keep call with the patches of d_dropped zeroed: reuse the copy (embed_reuse_kernel)
enum class Embed { fresh, keep, reuse };

}  // namespace

static int vit_forward_impl(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, int32_t B, void* stream, Embed embed) {
    if (!e || !d_images) return PNP_ERR_ARG;
    if (!e->w->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch) return fail(e, PNP_ERR_ARG, "batch %d out of range (max %d)", B, e->c.max_batch);
    hipStream_t s = (hipStream_t)stream;
    const int D = e->D, N = e->N, M = B * N, F = D * e->c.vit_mlp_ratio, bf = e->bf;
    const int ldv = e->c.max_batch * e->Npad;
    if (embed == Embed::reuse && d_dropped) {
        hipLaunchKernelGGL(embed_reuse_kernel, dim3(2048), dim3(256), 0, s, (const float*)e->x0, d_dropped, (const float*)e->w->patch_b,
                           (const float*)e->w->pos, e->x, M, N, D / 4);
        KCHK(e, launched());
    } else {
        KCHK(e, patchify(bf, d_images, d_dropped, e->patches, B, e->c.img_size, e->P, s));
        KCHK(e, cls_rows(e->w->cls, e->w->pos, e->x, B, N, D, s));
        {
            GemmArgs g = linear(e->patches, 768, e->w->patch_w, B * e->PP);
            g.bias = e->w->patch_b; g.resid = e->w->pos; g.ldr = D; g.out_f32 = e->x; g.ldo = D; g.row_div = e->PP;
            KCHK(e, egemm(e, g, s));
        }
        if (embed == Embed::keep)
            HIPCHK(e, hipMemcpyAsync(e->x0, e->x, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    const float scale = 1.0f / sqrtf(64.f);
    // split-bf16 ("bf16x3"): every Linear of the block is a wide-kernel launch on (hi, lo) bf16 operand pairs -- three bf16 MFMA
    // passes per product, fp32-class result; LayerNorm, the attention kernel and the GELU epilogue hand the next GEMM its
    // operand already split (the handles' lo halves, null in the other modes)
    const int ln = bf | e->x3;                   // LayerNorm writes bf16 for the pair too
    for (int l = 0; l < e->c.vit_depth; l++) {
        const VitLayerW& w = e->w->vit[l];
        KCHK(e, layernorm(ln, e->x, w.n1w, w.n1b, e->c.vit_ln_eps, M, D, nullptr, e->xn.hi, nullptr, nullptr, s, e->xn.lo));
        if (bf || e->x3) {   // q | k | v natural in one launch: [M, 3D] at the padded stride; the attention kernel transposes V on its LDS reads
            GemmArgs g = linear(e->xn, D, w.qkv_w, M);
            g.bias = w.qkv_b; g.out_t = e->qk.hi; g.out_lo = e->qk.lo; g.ldo_t = e->ldq;
            KCHK(e, egemm(e, g, s));
            if (e->x3)       // the split form of the bf16 kernel (vit_attn32_x3_kernel)
                KCHK(e, vit_attention_x3(e->qk.hi, e->qk.lo, e->ldq, D, e->ctx.hi, e->ctx.lo, B, e->c.vit_heads, N, scale, s));
            else
                KCHK(e, vit_attention(bf, e->qk.hi, e->ldq, D, (const char*)e->qk.hi + (size_t)2 * D * e->esz, e->ldq, e->Npad, e->ctx.hi,
                                      B, e->c.vit_heads, N, scale, s));
        } else {
            {   // q | k  natural: [M, 2D]
                GemmArgs g = linear(e->xn, D, w.qkv_w, M, 0, 2 * D);
                g.bias = w.qkv_b; g.out_t = e->qk.hi; g.ldo_t = 2 * D;
                KCHK(e, egemm(e, g, s));
            }
            {   // V^T: [D, B*Npad] = Wv . xn^T, token columns padded per image
                GemmArgs g = linear_t(e->xn, D, w.qkv_w, M, 2 * D, D);
                g.bias = w.qkv_b + 2 * D; g.bias_on_rows = 1; g.out_t = e->vt; g.ldo_t = ldv; g.col_div = N; g.col_pad = e->Npad;
                KCHK(e, egemm(e, g, s));
            }
            KCHK(e, vit_attention(bf, e->qk.hi, 2 * D, D, e->vt, ldv, e->Npad, e->ctx.hi, B, e->c.vit_heads, N, scale, s));
        }
        {
            GemmArgs g = linear(e->ctx, D, w.proj_w, M);
            g.bias = w.proj_b; g.resid = e->x; g.ldr = D; g.out_f32 = e->x; g.ldo = D;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, layernorm(ln, e->x, w.n2w, w.n2b, e->c.vit_ln_eps, M, D, nullptr, e->xn.hi, nullptr, nullptr, s, e->xn.lo));
        {
            GemmArgs g = linear(e->xn, D, w.fc1_w, M);
            g.bias = w.fc1_b; g.mode = GEMM_EPI_GELU; g.out_t = e->h1.hi; g.out_lo = e->h1.lo; g.ldo_t = F;
            KCHK(e, egemm(e, g, s));
        }
        {
            GemmArgs g = linear(e->h1, F, w.fc2_w, M);
            g.bias = w.fc2_b; g.resid = e->x; g.ldr = D; g.out_f32 = e->x; g.ldo = D;
            KCHK(e, egemm(e, g, s));
        }
    }
    KCHK(e, layernorm(ln, e->x, e->w->vnorm_w, e->w->vnorm_b, e->c.vit_ln_eps, M, D, e->emb32, e->embT.hi, nullptr, nullptr, s, e->embT.lo));
    return pnp_cross_kv(e, B, stream);
}
extern "C" int pnp_vit_forward(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, int32_t B, void* stream) {
    return vit_forward_impl(e, d_images, d_dropped, B, stream, Embed::fresh);
}

// encoder_hidden_states -> key / value of every text layer's cross-attention (B/med.py:208-211): the reference
// projects image_embeds once per layer inside BertSelfAttention.forward; here all 12 layers are projected in four
// launches (natural + transposed layouts) right after the ViT, from the compute-type copy of image_embeds.
extern "C" int pnp_cross_kv(pnp_engine* e, int32_t B, void* stream) {
    if (!e) return PNP_ERR_ARG;
    if (!e->w->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch) return fail(e, PNP_ERR_ARG, "batch %d out of range (max %d)", B, e->c.max_batch);
    hipStream_t s = (hipStream_t)stream;
    const int D = e->D, N = e->N, M = B * N;
    const int ldv = e->c.max_batch * e->Npad;
    const int H = e->H, TL = e->TL, SL = e->SL, nVn = TL - SL, nKt = TL - SL - 1;
    // K token-major and V^T feature-major of all layers: fp32 from the pair GEMM in bf16x3, the compute type otherwise
    auto out = [&](GemmArgs& g, void* p, int ld) {
        if (e->x3) { g.out_f32 = (float*)p; g.ldo = ld; }
        else { g.out_t = p; g.ldo_t = ld; }
    };
    {
        GemmArgs g = linear(e->embT, D, e->w->ck_w, M);
        g.bias = e->w->ck_b; out(g, e->Knat, TL * H);
        KCHK(e, egemm(e, g, s));
    }
    {
        GemmArgs g = linear_t(e->embT, D, e->w->cv_w, M);
        g.bias = e->w->cv_b; g.bias_on_rows = 1; out(g, e->Vt, ldv); g.col_div = N; g.col_pad = e->Npad;
        KCHK(e, egemm(e, g, s));
    }
    // V token-major of layers >= SL, K^T of layers > SL
    if (e->x3) {             // from V^T and from K token-major (see feat_to_tok_kernel)
        hipLaunchKernelGGL(feat_to_tok_kernel, dim3((nVn * H + 31) / 32, (N + 31) / 32, B), dim3(32, 8), 0, s,
                           (const float*)e->Vt + (size_t)SL * H * ldv, ldv, e->Npad, (float*)e->Vnat, nVn * H, N);
        KCHK(e, launched());
        if (nKt > 0) {
            hipLaunchKernelGGL(tok_to_feat_kernel, dim3((nKt * H + 31) / 32, (N + 31) / 32, B), dim3(32, 8), 0, s,
                               (const float*)e->Knat + (size_t)(SL + 1) * H, TL * H, (float*)e->Kt, ldv, e->Npad, nKt * H, N);
            KCHK(e, launched());
        }
        return PNP_OK;
    }
    {
        GemmArgs g = linear(e->embT, D, e->w->cv_w, M, SL * H, nVn * H);
        g.bias = e->w->cv_b + (size_t)SL * H; g.out_t = e->Vnat; g.ldo_t = nVn * H;
        KCHK(e, egemm(e, g, s));
    }
    if (nKt > 0) {
        GemmArgs g = linear_t(e->embT, D, e->w->ck_w, M, (SL + 1) * H, nKt * H);
        g.bias = e->w->ck_b + (size_t)(SL + 1) * H; g.bias_on_rows = 1; g.out_t = e->Kt; g.ldo_t = ldv; g.col_div = N; g.col_pad = e->Npad;
        KCHK(e, egemm(e, g, s));
    }
    return PNP_OK;
}

// One BERT layer of the text stack on the R = B * L rows in place (layer 0 reads h0, layer i the h_out of layer i - 1): the
// self-attention sub-layer, the cross-attention sub-layer over the image's K / V, the FFN.
//   cross = false: the text-only form -- no cross-attention sub-layer (the FFN reads a_out), and nothing is kept for the backward
//   self_in_place: the self-attention sub-layer's outputs of the previous call are valid (text_forward_impl's prefix reuse)
static int text_layer(pnp_engine* e, int i, const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, bool cross, bool self_in_place,
                      hipStream_t s) {
    const int H = e->H, I = e->I, TL = e->TL, R = B * L, bf = e->bf, N = e->N;
    const int ldv = e->c.max_batch * e->Npad;
    const TextLayerW& w = e->w->txt[i];
    TextLayerA& a = e->ta[i];
    const float* h = i ? e->ta[i - 1].h_out : e->h0;
    const void* hT = i ? e->ta[i - 1].h_outT : e->h0T;
    const bool keep_p = cross && i >= e->SL;                               // the attention probabilities of the stash layers
    auto keep = [&](float* p) -> float* { return cross ? p : nullptr; };   // the LayerNorm x-hat / rstd the backward reads
    if (!self_in_place) {
        {
            GemmArgs g = linear(hT, H, w.qkv_w, R);
            g.bias = w.qkv_b; g.out_t = a.qkv; g.ldo_t = 3 * H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, text_self_attn(bf, a.qkv, d_mask, ld, e->ctx_s, keep_p ? a.Ps : nullptr, e->dS, B, L, H, s));
        {
            GemmArgs g = linear(e->ctx_s, H, w.so_w, R);
            g.bias = w.so_b; g.resid = h; g.ldr = H; g.out_f32 = e->tmp; g.ldo = H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, layernorm(bf, e->tmp, w.sln_w, w.sln_b, e->c.txt_ln_eps, R, H, a.a_out, a.a_outT, keep(a.a_hat), keep(a.a_rstd), s));
    }
    const float* f = a.a_out;                    // the rows the FFN reads
    const void* fT = a.a_outT;
    if (cross) {
        {
            GemmArgs g = linear(a.a_outT, H, w.cq_w, R);
            g.bias = w.cq_b; g.out_t = a.qc; g.ldo_t = H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, xattn(bf, 0, (const char*)e->Knat + (size_t)i * H * e->esz, TL * H,
                      (const char*)e->Vt + (size_t)i * H * ldv * e->esz, ldv, e->Npad, a.qc, H, e->ctx_c, H,
                      keep_p ? a.Pc : nullptr, e->Nst, B, L, N, e->nh, s));
        {
            GemmArgs g = linear(e->ctx_c, H, w.co_w, R);
            g.bias = w.co_b; g.resid = a.a_out; g.ldr = H; g.out_f32 = e->tmp; g.ldo = H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, layernorm(bf, e->tmp, w.cln_w, w.cln_b, e->c.txt_ln_eps, R, H, a.c_out, a.c_outT, a.c_hat, a.c_rstd, s));
        f = a.c_out;
        fT = a.c_outT;
    }
    {
        GemmArgs g = linear(fT, H, w.i_w, R);
        g.bias = w.i_b; g.mode = GEMM_EPI_GELU; g.out_t = e->g; g.ldo_t = I;
        if (cross) { g.aux = a.u; g.ld_aux = I; }                          // the GELU pre-activation, for the backward
        KCHK(e, egemm(e, g, s));
    }
    {
        GemmArgs g = linear(e->g, I, w.o_w, R);
        g.bias = w.o_b; g.resid = f; g.ldr = H; g.out_f32 = e->tmp; g.ldo = H;
        KCHK(e, egemm(e, g, s));
    }
    KCHK(e, layernorm(bf, e->tmp, w.oln_w, w.oln_b, e->c.txt_ln_eps, R, H, a.h_out, a.h_outT, keep(a.o_hat), keep(a.o_rstd), s));
    return PNP_OK;
}

// reuse_prefix: the token ids / mask are those of the previous call on this engine (drop iterations 1..): the embeddings and the
// self-attention sub-layer of text layer 0 do not see the image -- their activations of the previous call are still in place
static int text_forward_impl(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t B, int32_t L,
                             float* d_logits, void* stream, bool reuse_prefix) {
    if (!e || !d_ids || !d_mask) return PNP_ERR_ARG;
    if (!e->w->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch || L < 5 || L > e->c.max_text_len || ld < L)
        return fail(e, PNP_ERR_ARG, "text batch %d x %d (ld %d) out of range (max %d x %d)", B, L, ld, e->c.max_batch, e->c.max_text_len);
    hipStream_t s = (hipStream_t)stream;
    const int H = e->H, TL = e->TL, R = B * L;
    e->acts_text_only = false;
    if (!reuse_prefix) {
        KCHK(e, text_embed(d_ids, ld, e->w->word, e->w->tpos, e->temb, B, L, H, e->c.enc_token_id, e->c.vocab, s));
        KCHK(e, layernorm(e->bf, e->temb, e->w->eln_w, e->w->eln_b, e->c.txt_ln_eps, R, H, e->h0, e->h0T, nullptr, nullptr, s));
    }
    for (int i = 0; i < TL; i++) {
        int r = text_layer(e, i, d_mask, ld, B, L, true, reuse_prefix && i == 0, s);
        if (r) return r;
    }
    KCHK(e, itm_head(e->ta[TL - 1].h_out, e->w->itm_w, e->w->itm_b, d_logits ? d_logits : e->logits_scratch, B, L, H, s));
    return PNP_OK;
}
extern "C" int pnp_text_forward_xattn(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t B,
                                      int32_t L, float* d_logits, void* stream) {
    return text_forward_impl(e, d_ids, d_mask, ld, B, L, d_logits, stream, false);
}

// BertModel.forward(mode="text") (B/med.py:565-568, 473): the text stack without its cross-attention sub-layers and without the
// [ENC] substitution, for T texts that need no image.  Runs in the multimodal pass's activation buffers (temb, h0, tmp, ctx_s, g and
// each layer's qkv / a_out / h_out with their compute-type copies; no stash is written), max_batch rows of text at a time, so what
// those buffers held for a GradCAM backward is gone: the kept layer and the backward are invalidated.  image_embeds
// and the cross K / V of the last pnp_vit_forward are not touched.
extern "C" int pnp_text_forward_text(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t T, int32_t L,
                                     float* d_hidden, void* stream) {
    if (!e || !d_ids || !d_mask) return PNP_ERR_ARG;
    if (T <= 0 || L < 2 || L > e->c.max_text_len || ld < L)
        return fail(e, PNP_ERR_ARG, "text batch %d x %d (ld %d) out of range (2 <= L <= %d, T > 0)", T, L, ld, e->c.max_text_len);
    if (!e->w->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    hipStream_t s = (hipStream_t)stream;
    const int H = e->H, TL = e->TL;
    e->grad_layer = -1;
    e->acts_text_only = true;
    for (int t0 = 0; t0 < T; t0 += e->c.max_batch) {
        const int B = T - t0 < e->c.max_batch ? T - t0 : e->c.max_batch, R = B * L;
        const int64_t* ids = d_ids + (size_t)t0 * ld;
        const int64_t* mask = d_mask + (size_t)t0 * ld;
        KCHK(e, text_embed(ids, ld, e->w->word, e->w->tpos, e->temb, B, L, H, -1, e->c.vocab, s));
        KCHK(e, layernorm(e->bf, e->temb, e->w->eln_w, e->w->eln_b, e->c.txt_ln_eps, R, H, e->h0, e->h0T, nullptr, nullptr, s));
        for (int i = 0; i < TL; i++) {
            int r = text_layer(e, i, mask, ld, B, L, false, false, s);
            if (r) return r;
        }
        if (d_hidden)
            HIPCHK(e, hipMemcpyAsync(d_hidden + (size_t)t0 * L * H, e->ta[TL - 1].h_out, (size_t)R * H * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
    }
    return PNP_OK;
}

// F.normalize(Linear(x), dim=-1) with vision_proj (which = 0) or text_proj (which = 1) (B/blip_image_text_matching.py:137-138,
// 158-159, 260-263): the Linear is one launch of the mode's GEMM (exact fp32 MFMA | split-bf16 with the fp32 rows split by the
// kernel | bf16 after a cast of the rows into the ViT's LayerNorm scratch) with fp32 output, then l2_normalize_rows in place.
extern "C" int pnp_project_normalize(pnp_engine* e, int32_t which, const float* d_x, int64_t row_stride, int32_t rows, float* d_out,
                                     void* stream) {
    if (!e || !d_x || !d_out) return PNP_ERR_ARG;
    if (which < 0 || which > 1) return fail(e, PNP_ERR_ARG, "which = %d: 0 (vision_proj) or 1 (text_proj)", which);
    if (rows <= 0) return fail(e, PNP_ERR_ARG, "rows = %d", rows);
    const int K = which == 0 ? e->D : e->H;
    if (row_stride < K || row_stride % 4 || row_stride > (int64_t)1 << 30)
        return fail(e, PNP_ERR_ARG, "row_stride %lld: a multiple of 4 elements, at least %d", (long long)row_stride, K);
    // the GEMM kernels address an operand by 32-bit byte offsets from its base
    if ((int64_t)rows * row_stride * 4 >= (int64_t)1 << 32)
        return fail(e, PNP_ERR_ARG, "rows %d x row_stride %lld: the input must span less than 4 GiB", rows, (long long)row_stride);
    if (!e->w->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    const Weight& w = e->w->proj_w[which];
    if (!w.p || !e->w->proj_b[which])
        return fail(e, PNP_ERR_STATE, "missing weight %s.weight (the state dict held no %s.weight / .bias)", kProj[which], kProj[which]);
    hipStream_t s = (hipStream_t)stream;
    const int E = e->w->proj_E[which];
    if (e->bf) {
        // bf16 operands: rows are cast into xn (free between ViT forwards), as many at a time as it holds
        size_t cap = (size_t)e->c.max_batch * e->N * e->D / K;
        cap = cap < 16384 ? cap : 16384;           // (and few enough for the generic tiles: the wide bf16 kernel has no such epilogue)
        for (size_t r0 = 0; r0 < (size_t)rows; r0 += cap) {
            const int n = (int)((size_t)rows - r0 < cap ? (size_t)rows - r0 : cap);
            KCHK(e, cast_rows_bf16(d_x + r0 * row_stride, (int)row_stride, e->xn.hi, n, K, s));
            GemmArgs g = linear(e->xn.hi, K, w, n);
            g.bias = e->w->proj_b[which]; g.out_f32 = d_out + r0 * E; g.ldo = E;
            KCHK(e, egemm(e, g, s));
        }
    } else {
        GemmArgs g = linear(d_x, (int)row_stride, w, rows);
        g.bias = e->w->proj_b[which]; g.out_f32 = d_out; g.ldo = E;
        KCHK(e, egemm(e, g, s));
    }
    KCHK(e, l2_normalize_rows(d_out, rows, E, 1e-12f, s));
    return PNP_OK;
}

extern "C" int pnp_xattn_grad(pnp_engine* e, int32_t B, int32_t L, void* stream) {
    return pnp_xattn_grad_layer(e, B, L, e ? e->SL : 0, stream);
}

extern "C" int pnp_xattn_grad_layer(pnp_engine* e, int32_t B, int32_t L, int32_t layer, void* stream) {
    if (!e) return PNP_ERR_ARG;
    if (!e->w->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch || L < 5 || L > e->c.max_text_len) return fail(e, PNP_ERR_ARG, "bad B/L");
    if (layer < e->SL || layer >= e->TL)
        return fail(e, PNP_ERR_ARG, "layer %d: cross-attention maps are kept for text layers %d..%d (stash_layer)", layer, e->SL, e->TL - 1);
    if (e->acts_text_only)
        return fail(e, PNP_ERR_STATE, "the text activations in place are those of pnp_text_forward_text: run pnp_text_forward_xattn first");
    hipStream_t s = (hipStream_t)stream;
    const int H = e->H, I = e->I, TL = e->TL, R = B * L, bf = e->bf, N = e->N, SL = e->SL;
    const int ldv = e->c.max_batch * e->Npad, nVn = TL - SL;
    e->grad_layer = layer;
    KCHK(e, itm_grad_seed(e->w->itm_w, e->dh, B, L, H, s));
    for (int i = TL - 1; i >= layer; i--) {
        const TextLayerW& w = e->w->txt[i];
        TextLayerA& a = e->ta[i];
        KCHK(e, layernorm_bwd(bf, e->dh, w.oln_w, a.o_hat, a.o_rstd, R, H, e->d_pre, e->d_preT, s));
        {   // dg = (d_pre . Wo2) * gelu'(u)
            GemmArgs g = linear(e->d_preT, H, w.o_wT, R);
            g.mode = GEMM_EPI_GELU_GRAD; g.aux = a.u; g.ld_aux = I; g.out_t = e->dg; g.ldo_t = I;
            KCHK(e, egemm(e, g, s));
        }
        {   // dc = d_pre + dg . Wi
            GemmArgs g = linear(e->dg, I, w.i_wT, R);
            g.resid = e->d_pre; g.ldr = H; g.out_f32 = e->dc; g.ldo = H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, layernorm_bwd(bf, e->dc, w.cln_w, a.c_hat, a.c_rstd, R, H, e->d_cpre, e->d_cpreT, s));
        {
            GemmArgs g = linear(e->d_cpreT, H, w.co_wT, R);
            g.out_t = e->dctxc; g.ldo_t = H;
            KCHK(e, egemm(e, g, s));
        }
        const char* vnat = (const char*)e->Vnat + (size_t)(i - SL) * H * e->esz;
        if (i == layer) {
            KCHK(e, xattn(bf, 2, vnat, nVn * H, nullptr, 0, e->Npad, e->dctxc, H, nullptr, 0, e->dPc, e->Nst, B, L, N, e->nh, s));
            break;
        }
        KCHK(e, xattn(bf, 1, vnat, nVn * H, (const char*)e->Kt + (size_t)(i - SL - 1) * H * ldv * e->esz, ldv, e->Npad,
                      e->dctxc, H, e->dqc, H, a.Pc, e->Nst, B, L, N, e->nh, s));
        {
            GemmArgs g = linear(e->dqc, H, w.cq_wT, R);
            g.resid = e->d_cpre; g.ldr = H; g.out_f32 = e->da; g.ldo = H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, layernorm_bwd(bf, e->da, w.sln_w, a.a_hat, a.a_rstd, R, H, e->d_apre, e->d_apreT, s));
        {
            GemmArgs g = linear(e->d_apreT, H, w.so_wT, R);
            g.out_f32 = e->dctx_s; g.ldo = H;
            KCHK(e, egemm(e, g, s));
        }
        KCHK(e, text_self_attn_bwd(bf, a.qkv, e->dctx_s, a.Ps, e->dS, e->dqkv, B, L, H, s));
        {
            GemmArgs g = linear(e->dqkv, 3 * H, w.qkv_wT, R);
            g.resid = e->d_apre; g.ldr = H; g.out_f32 = e->dh; g.ldo = H;
            KCHK(e, egemm(e, g, s));
        }
    }
    return PNP_OK;
}

extern "C" int pnp_gradcam_gather(pnp_engine* e, const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t head,
                                  float* d_out, void* stream) {
    if (!e || !d_mask || !d_out) return PNP_ERR_ARG;
    if (head < 0 || head >= e->nh) return fail(e, PNP_ERR_ARG, "head %d out of range", head);
    if (B <= 0 || B > e->c.max_batch || L < 5 || L > e->c.max_text_len || ld < L) return fail(e, PNP_ERR_ARG, "bad B/L/ld");
    if (e->grad_layer < 0) return fail(e, PNP_ERR_STATE, "call pnp_xattn_grad first");
    // P of the layer the last backward stopped at, and its dL/dP
    KCHK(e, gradcam_gather(e->ta[e->grad_layer].Pc, e->dPc, d_mask, ld, d_out, B, e->nh, head, L, e->Nst, e->PP, (hipStream_t)stream));
    return PNP_OK;
}

static int compute_gradcam_impl(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, const int64_t* d_ids,
                                const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t layer, int32_t head,
                                float* d_out, float* d_logits, void* stream, Embed embed) {
    int r = vit_forward_impl(e, d_images, d_dropped, B, stream, embed);
    if (r) return r;
    // drop iterations 1..: same captions as iteration 0 (Embed::reuse only comes from the drop loop; a stash layer of 0 keeps the
    // probabilities of layer 0's self-attention, which are in place as well)
    r = text_forward_impl(e, d_ids, d_mask, ld, B, L, d_logits, stream, embed == Embed::reuse);
    if (r) return r;
    r = pnp_xattn_grad_layer(e, B, L, layer, stream);
    if (r) return r;
    return pnp_gradcam_gather(e, d_mask, ld, B, L, head, d_out, stream);
}
extern "C" int pnp_compute_gradcam_layer(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, const int64_t* d_ids,
                                         const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t layer, int32_t head,
                                         float* d_out, float* d_logits, void* stream) {
    return compute_gradcam_impl(e, d_images, d_dropped, d_ids, d_mask, ld, B, L, layer, head, d_out, d_logits, stream, Embed::fresh);
}

extern "C" int pnp_compute_gradcam(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, const int64_t* d_ids,
                                   const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t head, float* d_out,
                                   float* d_logits, void* stream) {
    return pnp_compute_gradcam_layer(e, d_images, d_dropped, d_ids, d_mask, ld, B, L, e ? e->SL : 0, head, d_out, d_logits, stream);
}

extern "C" int pnp_drop_step(pnp_engine* e, const float* d_gradcam, float* d_g0, float* d_agg, uint8_t* d_dropped,
                             int32_t* d_picks, int32_t iter, int32_t B, int32_t T, int32_t npick, int32_t max_picks,
                             void* stream) {
    if (!e || !d_gradcam || !d_agg || !d_dropped || (npick > 0 && !d_picks)) return PNP_ERR_ARG;
    if (T < 4) return fail(e, PNP_ERR_ARG, "T=%d too short", T);
    KCHK(e, drop_step(d_gradcam, d_g0, d_agg, d_dropped, d_picks, iter, B, T, e->PP, npick, max_picks, (hipStream_t)stream));
    return PNP_OK;
}

extern "C" int pnp_drop_loop(pnp_engine* e, const float* d_images, const int64_t* d_ids, const int64_t* d_mask, int32_t ld,
                             int32_t B, int32_t L, int32_t head, int32_t drop_iter, int32_t npick, float* d_g0,
                             float* d_agg, int32_t* d_picks, float* d_logits, void* stream) {
    return pnp_drop_loop_layer(e, d_images, d_ids, d_mask, ld, B, L, e ? e->SL : 0, head, drop_iter, npick, d_g0, d_agg, d_picks,
                               d_logits, stream);
}

extern "C" int pnp_drop_loop_layer(pnp_engine* e, const float* d_images, const int64_t* d_ids, const int64_t* d_mask, int32_t ld,
                                   int32_t B, int32_t L, int32_t layer, int32_t head, int32_t drop_iter, int32_t npick, float* d_g0,
                                   float* d_agg, int32_t* d_picks, float* d_logits, void* stream) {
    if (!e || !d_images || !d_ids || !d_mask || !d_g0) return PNP_ERR_ARG;
    if (drop_iter < 1) return fail(e, PNP_ERR_ARG, "drop_iter must be >= 1");
    if (drop_iter == 1)   // PnP.py:565-575: single call, no aggregate
        return pnp_compute_gradcam_layer(e, d_images, nullptr, d_ids, d_mask, ld, B, L, layer, head, d_g0, d_logits, stream);
    if (!d_agg || !d_picks) return PNP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(e, hipMemsetAsync(e->dropped, 0, (size_t)B * e->PP, s));
    for (int it = 0; it < drop_iter; it++) {
        // the token embeddings of iteration 0 serve the later iterations (same images, more patches zeroed)
        // Embed::reuse is safe here and nowhere else: iterations >= 1 pass the arguments of iteration 0 within this one C call, no
        // other entry point of this engine can run in between, and a failed iteration returns
        int r = compute_gradcam_impl(e, d_images, e->dropped, d_ids, d_mask, ld, B, L, layer, head, e->G, d_logits, stream,
                                     it == 0 ? Embed::keep : Embed::reuse);
        if (r) return r;
        r = pnp_drop_step(e, e->G, d_g0, d_agg, e->dropped, d_picks, it, B, L - 1, npick, drop_iter * npick, stream);
        if (r) return r;
    }
    return PNP_OK;
}
