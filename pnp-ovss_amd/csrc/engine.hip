// The engine behind include/pnp_hip.h: owns weights + workspace on one MI355X, sequences the
// hand-written kernels of this directory on the caller's stream: lifetime, weights, model, introspection and the operator
// shims (the post-processing entry points are in post.hip; the state both share is engine.h).  Host logic, but for four small
// layout kernels (transpose_cast_kernel_f32, feat_to_tok_kernel, tok_to_feat_kernel, embed_reuse_kernel); every FLOP of the
// hot path is in the other .hip files.  No allocation / sync inside hot-path calls.
#include <cmath>
#include <cstring>
#include <utility>

#include "engine.h"

using namespace pnp;

namespace {

int alloc_act(pnp_engine* e, Act* a, size_t rows, size_t ld) {   // the pair's two bf16 arrays fill the bytes of the fp32 rows
    KCHK(e, dalloc_t(e, &a->hi, rows * ld));
    a->lo = e->x3 ? (char*)a->hi + rows * ld * 2 : nullptr;
    return PNP_OK;
}

bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

__global__ void transpose_cast_kernel_f32(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
    __shared__ float t[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int r = by + i, c = bx + threadIdx.x;
        t[i][threadIdx.x] = (r < rows && c < cols) ? in[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += 8) {
        const int c = bx + i, r = by + threadIdx.x;
        if (r < rows && c < cols) out[(size_t)c * rows + r] = t[threadIdx.x][i];
    }
}

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

int new_weight(pnp_engine* e, int rows, int cols, bool pair, Weight* w) {
    *w = Weight{nullptr, rows, cols, pair ? 2 : (int)e->esz, pair};
    return dalloc_t(e, &w->p, (size_t)rows * cols);      // a pair belongs to bf16x3, whose compute type is fp32
}
// fp32 [n, w.cols] staging -> rows r0 .. r0 + n of the device weight
int fill_weight(pnp_engine* e, const float* src32, const Weight& w, int r0, int n) {
    const size_t count = (size_t)n * w.cols;
    return w.pair ? split_f32(src32, w.hi(r0), w.lo(r0), count, 0) : cast_f32(e->bf, src32, w.hi(r0), count, 0);
}
// fp32 [rows, cols] staging -> device weight of the compute type, or a (hi | lo) pair (`pair`: bf16x3, weights of the wide
// GEMMs); transpose: the weight is the [cols, rows] transpose
int make_weight(pnp_engine* e, const float* src32, int rows, int cols, bool transpose, Weight* out, bool pair = false) {
    KCHK(e, new_weight(e, transpose ? cols : rows, transpose ? rows : cols, pair, out));
    const float* s = src32;
    float* tmp = nullptr;
    if (transpose) {
        HIPCHK(e, hipMalloc((void**)&tmp, (size_t)rows * cols * 4));
        hipLaunchKernelGGL(transpose_cast_kernel_f32, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, 0, src32, tmp,
                           rows, cols);
        s = tmp;
    }
    int r = transpose ? launched() : PNP_OK;
    if (r == PNP_OK) r = fill_weight(e, s, *out, 0, out->rows);
    hipError_t st = hipDeviceSynchronize();
    if (tmp) (void)hipFree(tmp);
    if (r != PNP_OK || st != hipSuccess) return fail(e, PNP_ERR_HIP, "weight conversion failed");
    return PNP_OK;
}

GemmArgs G_(const void* A, int lda, const void* B, int ldb, int M, int N, int K) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    return g;
}

// The launch of a Linear in the engine's mode, y[M, n] = a[M, K] . w[r0 .. r0 + n, K]^T (n = 0: the whole weight); the caller
// adds the epilogue.  A pair weight (bf16x3) meets either a pair activation, or one fp32 array whose rows the kernel splits
// (a_f32: the text side, gemm_nt_small_x3_kernel).
GemmArgs linear(const void* a, int lda, const Weight& w, int M, int r0 = 0, int n = 0) {
    GemmArgs g = G_(a, lda, w.hi(r0), w.cols, M, n ? n : w.rows, w.cols);
    g.B_lo = w.lo(r0);
    g.a_f32 = w.pair;
    return g;
}
GemmArgs linear(const Act& a, int lda, const Weight& w, int M, int r0 = 0, int n = 0) {
    GemmArgs g = linear(a.hi, lda, w, M, r0, n);
    g.A_lo = a.lo;
    g.a_f32 = w.pair && !a.lo;
    return g;
}
// the same product written feature-major, y^T[n, M] = w . a^T: the operands change places
GemmArgs linear_t(const Act& a, int lda, const Weight& w, int M, int r0 = 0, int n = 0) {
    GemmArgs g = linear(a, lda, w, M, r0, n);
    std::swap(g.A, g.B); std::swap(g.A_lo, g.B_lo); std::swap(g.lda, g.ldb); std::swap(g.M, g.N);
    return g;
}

// every GEMM of an engine goes through here: the launch is timed into the engine's own ring when profiling is on.  gemm_nt
// takes the bf16 kernels by itself when an operand is a pair
int egemm(pnp_engine* e, GemmArgs g, hipStream_t s) {
    g.prof = e->gemm_prof;
    g.sk = e->sk_ws.part ? &e->sk_ws : nullptr;
    return gemm_nt(e->bf, g, s);
}

}  // namespace

// =========================================================================================== lifetime

extern "C" size_t pnp_workspace_bytes(const pnp_config* c) {
    if (!c) return 0;
    const size_t es = c->compute_bf16 == 1 ? 2 : 4;
    const size_t P = c->img_size / c->patch, N = P * P + 1, Npad = (N + 63) / 64 * 64, D = c->vit_dim, H = c->txt_hidden,
                 I = c->txt_inter, TL = c->txt_layers, B = c->max_batch, L = c->max_text_len;
    const size_t M = B * N, R = B * L;
    size_t w = (size_t)c->vit_depth * (12 * D * D) * es + TL * (4 * H * H + 2 * H * D + 2 * H * I) * es * 2 +
               ((size_t)c->vocab + c->max_pos) * H * 4 + 256 * (D + H) * es + 2 * 256 * 4;      // (incl. the optional ITC projections)
    size_t a = M * (768 + D * 2 + 3 * D + 64 + D + 4 * D) * es + M * D * 12 + D * B * Npad * es + M * TL * H * es * 2 +
               2 * TL * H * B * Npad * es;            // (incl. the padded q|k|v rows and the drop loop's copy of the token embeddings)
    size_t t = TL * (R * (3 * H + 2 * H) * es + R * (H * 8 + I) * 4 + B * (H / 64) * L * (L + Npad) * 4) + R * I * (4 + es) * 2 +
               R * H * 64;
    return w + a + t + (64u << 20);
}

extern "C" const char* pnp_last_error(const pnp_engine* e) { return e ? e->err : "null engine"; }

extern "C" void pnp_destroy(pnp_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->c.device);
    (void)hipDeviceSynchronize();
    for (void* p : e->allocs) (void)hipFree(p);
    for (auto& b : e->staging) if (b.p) (void)hipFree(b.p);
    if (e->gemm_prof) {
        for (int i = 0; i < e->gemm_prof->created; i++) {
            (void)hipEventDestroy(e->gemm_prof->ev0[i]);
            (void)hipEventDestroy(e->gemm_prof->ev1[i]);
        }
        delete e->gemm_prof;
    }
    for (hipEvent_t ev : e->crf_prof.ev0) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->crf_prof.ev1) (void)hipEventDestroy(ev);
    streamk_ws_destroy(&e->sk_ws);
    delete e;
}

static int create_impl(const pnp_config* cfg, pnp_engine* donor, pnp_engine** out) {
    if (!cfg || !out) return PNP_ERR_ARG;
    pnp_engine* e = new pnp_engine();
    *out = e;
    e->c = *cfg;
    if (donor) {
        const pnp_config& d = donor->c;
        if (!donor->finalized) return fail(e, PNP_ERR_STATE, "pnp_create_shared: the donor's weights are not finalized");
        if (d.device != cfg->device || d.compute_bf16 != cfg->compute_bf16 || d.img_size != cfg->img_size || d.patch != cfg->patch ||
            d.vit_dim != cfg->vit_dim || d.vit_depth != cfg->vit_depth || d.vit_heads != cfg->vit_heads ||
            d.vit_mlp_ratio != cfg->vit_mlp_ratio || d.txt_hidden != cfg->txt_hidden || d.txt_layers != cfg->txt_layers ||
            d.txt_heads != cfg->txt_heads || d.txt_inter != cfg->txt_inter || d.vocab != cfg->vocab || d.max_pos != cfg->max_pos ||
            d.vit_ln_eps != cfg->vit_ln_eps || d.txt_ln_eps != cfg->txt_ln_eps)
            return fail(e, PNP_ERR_ARG, "pnp_create_shared: device, compute mode and model geometry must equal the donor's");
        if (cfg->stash_layer < d.stash_layer)
            return fail(e, PNP_ERR_ARG, "pnp_create_shared: stash_layer %d below the donor's %d (its transposed backward weights "
                        "exist for layers >= %d only)", cfg->stash_layer, d.stash_layer, d.stash_layer);
    }
    const pnp_config& c = e->c;
    if (c.compute_bf16 < 0 || c.compute_bf16 > 2) return fail(e, PNP_ERR_ARG, "compute_bf16 must be 0 (fp32), 1 (bf16) or 2 (split-bf16)");
    e->bf = c.compute_bf16 == 1 ? 1 : 0;
    e->x3 = c.compute_bf16 == 2 ? 1 : 0;
    e->esz = e->bf ? 2 : 4;
    if (c.patch != 16) return fail(e, PNP_ERR_ARG, "patch must be 16");
    if (c.img_size % 16 || c.img_size <= 0) return fail(e, PNP_ERR_ARG, "img_size must be a positive multiple of 16");
    if (c.vit_dim != c.vit_heads * 64 || c.txt_hidden != c.txt_heads * 64)
        return fail(e, PNP_ERR_ARG, "head_dim must be 64 (vit_dim=%d heads=%d, txt_hidden=%d heads=%d)", c.vit_dim,
                    c.vit_heads, c.txt_hidden, c.txt_heads);
    if (c.vit_dim % 128 || c.txt_hidden % 128 || c.txt_inter % 128 || (c.vit_dim * c.vit_mlp_ratio) % 128)
        return fail(e, PNP_ERR_ARG, "widths must be multiples of 128");
    if (c.vit_dim > 1024 || c.txt_hidden > 1024) return fail(e, PNP_ERR_ARG, "LayerNorm width > 1024 unsupported");
    if (c.max_text_len < 5 || c.max_text_len > 512 || c.max_text_len > c.max_pos)
        return fail(e, PNP_ERR_ARG, "max_text_len must be in [5, min(512, max_pos = %d)]", c.max_pos);
    if (c.stash_layer < 0 || c.stash_layer >= c.txt_layers) return fail(e, PNP_ERR_ARG, "stash_layer out of range");
    if (c.max_batch <= 0) return fail(e, PNP_ERR_ARG, "max_batch must be positive");
    HIPCHK(e, hipSetDevice(c.device));
    e->P = c.img_size / 16;
    e->PP = e->P * e->P;
    e->N = e->PP + 1;
    e->Npad = (e->N + 63) / 64 * 64;
    e->Nst = e->Npad;
    e->D = c.vit_dim;
    e->H = c.txt_hidden;
    e->I = c.txt_inter;
    e->TL = c.txt_layers;
    e->nh = c.txt_heads;
    e->SL = c.stash_layer;
    if ((e->N + 15) / 16 > 160) return fail(e, PNP_ERR_ARG, "too many image tokens (%d) for the cross-attention kernel", e->N);
    const size_t B = c.max_batch, M = B * e->N, D = e->D, H = e->H, I = e->I, L = c.max_text_len, R = B * L, TL = e->TL;
    const size_t ldv = B * e->Npad;
    e->vit.resize(c.vit_depth);
    e->txt.resize(TL);
    e->ta.resize(TL);
    if (e->x3) {                               // one 256 KB partial-tile slot + one flag per CU (64 MB): not shared between engines
        const int n_cu = device_cu_count();
        if (!n_cu || streamk_ws_create(&e->sk_ws, n_cu) != PNP_OK) return fail(e, PNP_ERR_HIP, "stream-K workspace allocation failed");
        e->alloc_bytes += (size_t)n_cu * 256 * 256 * 4;
    }
    // activations
    KCHK(e, dalloc_t(e, &e->patches, B * e->PP * 768));
    KCHK(e, dalloc(e, &e->x, M * D));
    KCHK(e, dalloc(e, &e->x0, M * D));
    KCHK(e, alloc_act(e, &e->xn, M, D));
    // bf16 / split-bf16 modes: fused q|k|v rows at a stride of 3D + 64 elements; fp32 mode: q|k rows (v goes to vt).
    // The pad matters: an attention K / V tile is 64 rows x 128 B at the row stride, and at 6144 B (3D bf16, D = 1024) those
    // rows crowd a few L2 channels -- 151 us per launch against 136-138 us at 6272 ... 6656 B (tools/attn_ld_probe.py)
    e->ldq = 3 * (int)D + 64;
    KCHK(e, alloc_act(e, &e->qk, M, e->ldq));
    KCHK(e, dalloc_t(e, &e->vt, D * ldv, true));
    KCHK(e, alloc_act(e, &e->ctx, M, D));
    KCHK(e, alloc_act(e, &e->h1, M, D * c.vit_mlp_ratio));
    KCHK(e, alloc_act(e, &e->embT, M, D));
    KCHK(e, dalloc(e, &e->emb32, M * D));
    const int nVn = e->TL - e->SL, nKt = e->TL - e->SL - 1;
    KCHK(e, dalloc_t(e, &e->Knat, M * TL * H));
    KCHK(e, dalloc_t(e, &e->Vnat, M * (size_t)nVn * H));
    KCHK(e, dalloc_t(e, &e->Vt, TL * H * ldv, true));
    if (nKt > 0) KCHK(e, dalloc_t(e, &e->Kt, (size_t)nKt * H * ldv, true));
    KCHK(e, dalloc(e, &e->temb, R * H));
    KCHK(e, dalloc(e, &e->h0, R * H));
    KCHK(e, dalloc_t(e, &e->h0T, R * H));
    KCHK(e, dalloc(e, &e->tmp, R * H));
    KCHK(e, dalloc_t(e, &e->ctx_s, R * H));
    KCHK(e, dalloc_t(e, &e->ctx_c, R * H));
    KCHK(e, dalloc_t(e, &e->g, R * I));
    for (size_t i = 0; i < TL; i++) {
        TextLayerA& a = e->ta[i];
        KCHK(e, dalloc_t(e, &a.qkv, R * 3 * H));
        KCHK(e, dalloc(e, &a.a_hat, R * H));
        KCHK(e, dalloc(e, &a.a_rstd, R));
        KCHK(e, dalloc(e, &a.a_out, R * H));
        KCHK(e, dalloc_t(e, &a.a_outT, R * H));
        KCHK(e, dalloc_t(e, &a.qc, R * H));
        KCHK(e, dalloc(e, &a.c_hat, R * H));
        KCHK(e, dalloc(e, &a.c_rstd, R));
        KCHK(e, dalloc(e, &a.c_out, R * H));
        KCHK(e, dalloc_t(e, &a.c_outT, R * H));
        KCHK(e, dalloc(e, &a.u, R * I));
        KCHK(e, dalloc(e, &a.o_hat, R * H));
        KCHK(e, dalloc(e, &a.o_rstd, R));
        KCHK(e, dalloc(e, &a.h_out, R * H));
        KCHK(e, dalloc_t(e, &a.h_outT, R * H));
        if ((int)i >= e->SL) {
            KCHK(e, dalloc(e, &a.Ps, B * e->nh * L * L));
            KCHK(e, dalloc(e, &a.Pc, B * e->nh * L * (size_t)e->Nst, true));
        }
    }
    KCHK(e, dalloc(e, &e->dh, R * H));
    KCHK(e, dalloc(e, &e->d_pre, R * H));
    KCHK(e, dalloc_t(e, &e->d_preT, R * H));
    KCHK(e, dalloc_t(e, &e->dg, R * I));
    KCHK(e, dalloc(e, &e->dc, R * H));
    KCHK(e, dalloc(e, &e->d_cpre, R * H));
    KCHK(e, dalloc_t(e, &e->d_cpreT, R * H));
    KCHK(e, dalloc_t(e, &e->dctxc, R * H));
    KCHK(e, dalloc_t(e, &e->dqc, R * H));
    KCHK(e, dalloc(e, &e->da, R * H));
    KCHK(e, dalloc(e, &e->d_apre, R * H));
    KCHK(e, dalloc_t(e, &e->d_apreT, R * H));
    KCHK(e, dalloc(e, &e->dctx_s, R * H));
    KCHK(e, dalloc(e, &e->dS, B * e->nh * L * L));
    KCHK(e, dalloc(e, &e->dPc, B * e->nh * L * (size_t)e->Nst, true));
    KCHK(e, dalloc_t(e, &e->dqkv, R * 3 * H));
    KCHK(e, dalloc(e, &e->G, B * L * (size_t)e->PP));
    KCHK(e, dalloc(e, &e->dropped, B * (size_t)e->PP, true));
    KCHK(e, dalloc(e, &e->logits_scratch, B * 2));
    if (donor) {
        // weights: the donor's device copies (read-only after finalize); this engine owns activations and workspace only
        e->wstore = donor->wstore;
        e->shares_weights = true;
        e->cls = donor->cls; e->pos = donor->pos; e->patch_b = donor->patch_b; e->vnorm_w = donor->vnorm_w; e->vnorm_b = donor->vnorm_b;
        e->word = donor->word; e->tpos = donor->tpos; e->eln_w = donor->eln_w; e->eln_b = donor->eln_b;
        e->itm_w = donor->itm_w; e->itm_b = donor->itm_b; e->ck_b = donor->ck_b; e->cv_b = donor->cv_b;
        e->patch_w = donor->patch_w; e->ck_w = donor->ck_w; e->cv_w = donor->cv_w;
        e->vit = donor->vit;
        e->txt = donor->txt;
        for (int i = 0; i < 2; i++) { e->proj_w[i] = donor->proj_w[i]; e->proj_b[i] = donor->proj_b[i]; e->proj_E[i] = donor->proj_E[i]; }
        e->finalized = true;
        return PNP_OK;
    }
    e->wstore = std::make_shared<WeightStore>();
    e->wstore->device = c.device;
    e->to_store = true;
    // small fp32 params
    KCHK(e, dalloc(e, &e->cls, D));
    KCHK(e, dalloc(e, &e->pos, (size_t)e->N * D));
    KCHK(e, dalloc(e, &e->patch_b, D));
    KCHK(e, dalloc(e, &e->vnorm_w, D));
    KCHK(e, dalloc(e, &e->vnorm_b, D));
    KCHK(e, dalloc(e, &e->word, (size_t)c.vocab * H));
    KCHK(e, dalloc(e, &e->tpos, (size_t)c.max_pos * H));
    KCHK(e, dalloc(e, &e->eln_w, H));
    KCHK(e, dalloc(e, &e->eln_b, H));
    KCHK(e, dalloc(e, &e->itm_w, 2 * H));
    KCHK(e, dalloc(e, &e->itm_b, 2));
    KCHK(e, dalloc(e, &e->ck_b, TL * H));
    KCHK(e, dalloc(e, &e->cv_b, TL * H));
    for (auto& v : e->vit) {
        KCHK(e, dalloc(e, &v.n1w, D)); KCHK(e, dalloc(e, &v.n1b, D)); KCHK(e, dalloc(e, &v.n2w, D)); KCHK(e, dalloc(e, &v.n2b, D));
        KCHK(e, dalloc(e, &v.qkv_b, 3 * D)); KCHK(e, dalloc(e, &v.proj_b, D));
        KCHK(e, dalloc(e, &v.fc1_b, D * c.vit_mlp_ratio)); KCHK(e, dalloc(e, &v.fc2_b, D));
    }
    for (auto& t : e->txt) {
        KCHK(e, dalloc(e, &t.qkv_b, 3 * H)); KCHK(e, dalloc(e, &t.so_b, H)); KCHK(e, dalloc(e, &t.sln_w, H)); KCHK(e, dalloc(e, &t.sln_b, H));
        KCHK(e, dalloc(e, &t.cq_b, H)); KCHK(e, dalloc(e, &t.co_b, H)); KCHK(e, dalloc(e, &t.cln_w, H)); KCHK(e, dalloc(e, &t.cln_b, H));
        KCHK(e, dalloc(e, &t.i_b, I)); KCHK(e, dalloc(e, &t.o_b, H)); KCHK(e, dalloc(e, &t.oln_w, H)); KCHK(e, dalloc(e, &t.oln_b, H));
    }
    e->to_store = false;
    return PNP_OK;
}
extern "C" int pnp_create(const pnp_config* cfg, pnp_engine** out) { return create_impl(cfg, nullptr, out); }
extern "C" int pnp_create_shared(const pnp_config* cfg, pnp_engine* donor, pnp_engine** out) {
    if (!donor) return PNP_ERR_ARG;
    return create_impl(cfg, donor, out);
}

// =========================================================================================== weights

namespace {

// One tensor of the reference state dict and where it goes.  The three lists below (top level, ViT block, text layer) are the
// only place that names the keys: pnp_load_weight resolves a name through them, pnp_finalize_weights walks them to see that
// everything arrived.
struct Key {
    const char* name = "";
    float* small = nullptr;    // direct fp32 destination (biases, LN, embeddings); null: a GEMM weight, staged fp32 until finalize
    size_t small_off = 0;      // element offset inside `small`
    int rows = 1, cols = 0;
    int id = 0;                // GEMM weight: its index in finalize's array of staged pointers (the enums below)
};
Key small(const char* name, float* p, int count, size_t off = 0) { return {name, p, off, 1, count, 0}; }
Key gemm(const char* name, int id, int rows, int cols) { return {name, nullptr, 0, rows, cols, id}; }

enum { W_PATCH };
enum { W_QKV, W_PROJ, W_FC1, W_FC2 };
enum { W_Q, W_K, W_V, W_SO, W_CQ, W_CK, W_CV, W_CO, W_I, W_O, W_MAX };

std::vector<Key> top_keys(pnp_engine* e) {
    const int D = e->D, H = e->H;
    return {small("visual_encoder.cls_token", e->cls, D),
            small("visual_encoder.pos_embed", e->pos, e->N * D),
            gemm("visual_encoder.patch_embed.proj.weight", W_PATCH, D, 768),
            small("visual_encoder.patch_embed.proj.bias", e->patch_b, D),
            small("visual_encoder.norm.weight", e->vnorm_w, D),
            small("visual_encoder.norm.bias", e->vnorm_b, D),
            small("text_encoder.embeddings.word_embeddings.weight", e->word, e->c.vocab * H),
            small("text_encoder.embeddings.position_embeddings.weight", e->tpos, e->c.max_pos * H),
            small("text_encoder.embeddings.LayerNorm.weight", e->eln_w, H),
            small("text_encoder.embeddings.LayerNorm.bias", e->eln_b, H),
            small("itm_head.weight", e->itm_w, 2 * H),
            small("itm_head.bias", e->itm_b, 2)};
}
const char* const kVitPrefix = "visual_encoder.blocks.";
std::vector<Key> vit_keys(pnp_engine* e, int li) {
    VitLayerW& v = e->vit[li];
    const int D = e->D, F = D * e->c.vit_mlp_ratio;
    return {small("norm1.weight", v.n1w, D),       small("norm1.bias", v.n1b, D),
            gemm("attn.qkv.weight", W_QKV, 3 * D, D),   small("attn.qkv.bias", v.qkv_b, 3 * D),
            gemm("attn.proj.weight", W_PROJ, D, D),     small("attn.proj.bias", v.proj_b, D),
            small("norm2.weight", v.n2w, D),       small("norm2.bias", v.n2b, D),
            gemm("mlp.fc1.weight", W_FC1, F, D),        small("mlp.fc1.bias", v.fc1_b, F),
            gemm("mlp.fc2.weight", W_FC2, D, F),        small("mlp.fc2.bias", v.fc2_b, D)};
}
const char* const kTextPrefix = "text_encoder.encoder.layer.";
std::vector<Key> text_keys(pnp_engine* e, int li) {
    TextLayerW& t = e->txt[li];
    const int D = e->D, H = e->H, I = e->I;
    const size_t l = (size_t)li * H;               // this layer's part of the layer-major cross K / V biases
    return {gemm("attention.self.query.weight", W_Q, H, H),            small("attention.self.query.bias", t.qkv_b, H, 0),
            gemm("attention.self.key.weight", W_K, H, H),              small("attention.self.key.bias", t.qkv_b, H, H),
            gemm("attention.self.value.weight", W_V, H, H),            small("attention.self.value.bias", t.qkv_b, H, 2 * H),
            gemm("attention.output.dense.weight", W_SO, H, H),         small("attention.output.dense.bias", t.so_b, H),
            small("attention.output.LayerNorm.weight", t.sln_w, H),    small("attention.output.LayerNorm.bias", t.sln_b, H),
            gemm("crossattention.self.query.weight", W_CQ, H, H),      small("crossattention.self.query.bias", t.cq_b, H),
            gemm("crossattention.self.key.weight", W_CK, H, D),        small("crossattention.self.key.bias", e->ck_b, H, l),
            gemm("crossattention.self.value.weight", W_CV, H, D),      small("crossattention.self.value.bias", e->cv_b, H, l),
            gemm("crossattention.output.dense.weight", W_CO, H, H),    small("crossattention.output.dense.bias", t.co_b, H),
            small("crossattention.output.LayerNorm.weight", t.cln_w, H), small("crossattention.output.LayerNorm.bias", t.cln_b, H),
            gemm("intermediate.dense.weight", W_I, I, H),              small("intermediate.dense.bias", t.i_b, I),
            gemm("output.dense.weight", W_O, H, I),                    small("output.dense.bias", t.o_b, H),
            small("output.LayerNorm.weight", t.oln_w, H),              small("output.LayerNorm.bias", t.oln_b, H)};
}

bool find_key(const std::vector<Key>& keys, const char* name, Key& out) {
    for (const Key& k : keys)
        if (!strcmp(k.name, name)) {
            out = k;
            return true;
        }
    return false;
}

// resolve a reference state-dict key
bool resolve(pnp_engine* e, const std::string& n, Key& s) {
    int li = -1;
    char rest[128];
    auto layer_of = [&](const char* prefix, int depth) {      // "<prefix><li>.<rest>" with li < depth
        const size_t len = strlen(prefix);
        return n.compare(0, len, prefix) == 0 && sscanf(n.c_str() + len, "%d.%127s", &li, rest) == 2 && li >= 0 && li < depth;
    };
    if (layer_of(kVitPrefix, e->c.vit_depth)) return find_key(vit_keys(e, li), rest, s);
    if (layer_of(kTextPrefix, e->TL)) return find_key(text_keys(e, li), rest, s);
    return find_key(top_keys(e), n.c_str(), s);
}

// the optional ITC projections: 1 = `name` is one of the four tensors (staged like a GEMM weight until finalize), 0 = it is
// not, < 0 = its shape contradicts the model.  The embedding width E is the weight's first dimension.
const char* const kProj[2] = {"vision_proj", "text_proj"};
int resolve_proj(pnp_engine* e, const std::string& n, const int64_t* shape, int ndim, Key& s) {
    int which = -1;
    bool bias = false;
    for (int i = 0; i < 2; i++) {
        if (n == std::string(kProj[i]) + ".weight") which = i;
        if (n == std::string(kProj[i]) + ".bias") which = i, bias = true;
    }
    if (which < 0) return 0;
    const int K = which == 0 ? e->D : e->H;
    if (ndim != (bias ? 1 : 2) || (!bias && shape[1] != K))
        return fail(e, PNP_ERR_ARG, "%s: expected %s, second dimension %d", n.c_str(), bias ? "a vector" : "a matrix", K);
    const int64_t E = shape[0];
    if (E <= 0 || E > 1024 || E % 64) return fail(e, PNP_ERR_ARG, "%s: embedding width %lld must be a multiple of 64 up to 1024", n.c_str(), (long long)E);
    if (e->proj_E[which] && e->proj_E[which] != (int)E)
        return fail(e, PNP_ERR_ARG, "%s: %lld rows, but the other tensor of this projection has %d", n.c_str(), (long long)E, e->proj_E[which]);
    e->proj_E[which] = (int)E;
    s.rows = (int)E;
    s.cols = bias ? 1 : K;
    return 1;
}

const float* staged(pnp_engine* e, const std::string& n) {
    auto it = e->named.find("stage:" + n);
    return it == e->named.end() ? nullptr : (const float*)it->second.p;
}

// every tensor of a family must have arrived; st[id] <- the fp32 staging of its GEMM weights
int collect(pnp_engine* e, const std::string& prefix, const std::vector<Key>& keys, const float** st) {
    for (const Key& k : keys) {
        const std::string n = prefix + k.name;
        if (k.small ? !e->loaded.count(n) : !(st[k.id] = staged(e, n))) return fail(e, PNP_ERR_STATE, "missing weight %s", n.c_str());
    }
    return PNP_OK;
}

}  // namespace

extern "C" int pnp_load_weight(pnp_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim,
                               int32_t on_device) {
    if (!e || !name || !data || !shape) return PNP_ERR_ARG;
    if (e->shares_weights) return fail(e, PNP_ERR_STATE, "this engine uses a donor's weights (pnp_create_shared)");
    if (e->finalized) return fail(e, PNP_ERR_STATE, "weights already finalized");
    HIPCHK(e, hipSetDevice(e->c.device));
    Key s;
    const int pj = resolve_proj(e, name, shape, ndim, s);
    if (pj < 0) return pj;
    if (!pj && !resolve(e, name, s)) return PNP_OK;   // strict=False: not a tensor of this path
    size_t count = 1;
    for (int i = 0; i < ndim; i++) count *= (size_t)shape[i];
    if (count != (size_t)s.rows * s.cols) return fail(e, PNP_ERR_ARG, "%s: expected %d elements, got %zu", name, s.rows * s.cols, count);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (s.small) {
        HIPCHK(e, hipMemcpy(s.small + s.small_off, data, count * 4, kind));
    } else {
        Buf b;
        b.bytes = count * 4;
        HIPCHK(e, hipMalloc(&b.p, b.bytes));
        HIPCHK(e, hipMemcpy(b.p, data, b.bytes, kind));
        e->staging.push_back(b);
        e->named[std::string("stage:") + name] = b;
    }
    e->loaded[name] = true;
    return PNP_OK;
}

extern "C" int pnp_finalize_weights(pnp_engine* e) {
    if (!e) return PNP_ERR_ARG;
    if (e->finalized) return PNP_OK;
    HIPCHK(e, hipSetDevice(e->c.device));
    e->to_store = true;                        // everything allocated from here to the end of the call is a weight
    struct StoreOff { pnp_engine* e; ~StoreOff() { e->to_store = false; } } store_off{e};
    const int D = e->D, H = e->H, I = e->I, TL = e->TL, F = D * e->c.vit_mlp_ratio;
    const float* st[W_MAX];
    if (int r = collect(e, "", top_keys(e), st)) return r;
    KCHK(e, make_weight(e, st[W_PATCH], D, 768, false, &e->patch_w));
    for (int i = 0; i < e->c.vit_depth; i++) {
        VitLayerW& v = e->vit[i];
        if (int r = collect(e, kVitPrefix + std::to_string(i) + ".", vit_keys(e, i), st)) return r;
        KCHK(e, make_weight(e, st[W_QKV], 3 * D, D, false, &v.qkv_w, e->x3));
        KCHK(e, make_weight(e, st[W_PROJ], D, D, false, &v.proj_w, e->x3));
        KCHK(e, make_weight(e, st[W_FC1], F, D, false, &v.fc1_w, e->x3));
        KCHK(e, make_weight(e, st[W_FC2], D, F, false, &v.fc2_w, e->x3));
    }
    // cross-attention K / V weights of all layers, layer-major, so one GEMM projects every layer
    KCHK(e, new_weight(e, TL * H, D, e->x3, &e->ck_w));
    KCHK(e, new_weight(e, TL * H, D, e->x3, &e->cv_w));
    for (int i = 0; i < TL; i++) {
        TextLayerW& t = e->txt[i];
        if (int r = collect(e, kTextPrefix + std::to_string(i) + ".", text_keys(e, i), st)) return r;
        // fused self q|k|v [3H, H]
        float* fused = nullptr;
        HIPCHK(e, hipMalloc((void**)&fused, (size_t)3 * H * H * 4));
        HIPCHK(e, hipMemcpy(fused, st[W_Q], (size_t)H * H * 4, hipMemcpyDeviceToDevice));
        HIPCHK(e, hipMemcpy(fused + (size_t)H * H, st[W_K], (size_t)H * H * 4, hipMemcpyDeviceToDevice));
        HIPCHK(e, hipMemcpy(fused + (size_t)2 * H * H, st[W_V], (size_t)H * H * 4, hipMemcpyDeviceToDevice));
        int r = make_weight(e, fused, 3 * H, H, false, &t.qkv_w, e->x3);
        if (r == PNP_OK && i > e->SL) r = make_weight(e, fused, 3 * H, H, true, &t.qkv_wT, e->x3);
        (void)hipFree(fused);
        if (r != PNP_OK) return r;
        KCHK(e, make_weight(e, st[W_SO], H, H, false, &t.so_w, e->x3));
        KCHK(e, make_weight(e, st[W_CQ], H, H, false, &t.cq_w, e->x3));
        KCHK(e, make_weight(e, st[W_CO], H, H, false, &t.co_w, e->x3));
        KCHK(e, make_weight(e, st[W_I], I, H, false, &t.i_w, e->x3));
        KCHK(e, make_weight(e, st[W_O], H, I, false, &t.o_w, e->x3));
        KCHK(e, fill_weight(e, st[W_CK], e->ck_w, i * H, H));
        KCHK(e, fill_weight(e, st[W_CV], e->cv_w, i * H, H));
        if (i >= e->SL) {
            KCHK(e, make_weight(e, st[W_O], H, I, true, &t.o_wT, e->x3));      // [I][H]
            KCHK(e, make_weight(e, st[W_I], I, H, true, &t.i_wT, e->x3));      // [H][I]
            KCHK(e, make_weight(e, st[W_CO], H, H, true, &t.co_wT, e->x3));
        }
        if (i > e->SL) {
            KCHK(e, make_weight(e, st[W_CQ], H, H, true, &t.cq_wT, e->x3));
            KCHK(e, make_weight(e, st[W_SO], H, H, true, &t.so_wT, e->x3));
        }
    }
    // the optional ITC projections: converted like every other Linear weight when weight and bias both arrived
    for (int i = 0; i < 2; i++) {
        const float *w = staged(e, std::string(kProj[i]) + ".weight"), *bs = staged(e, std::string(kProj[i]) + ".bias");
        if (!w || !bs) {
            e->proj_E[i] = 0;
            continue;
        }
        KCHK(e, make_weight(e, w, e->proj_E[i], i == 0 ? D : H, false, &e->proj_w[i], e->x3));
        KCHK(e, dalloc(e, &e->proj_b[i], (size_t)e->proj_E[i]));
        HIPCHK(e, hipMemcpy(e->proj_b[i], bs, (size_t)e->proj_E[i] * 4, hipMemcpyDeviceToDevice));
    }
    HIPCHK(e, hipDeviceSynchronize());
    for (auto& b : e->staging) if (b.p) (void)hipFree(b.p);
    e->staging.clear();
    for (auto it = e->named.begin(); it != e->named.end();) {
        if (it->first.rfind("stage:", 0) == 0) it = e->named.erase(it);
        else ++it;
    }
    e->finalized = true;
    return PNP_OK;
}

// =========================================================================================== model

// embed: 0 = compute the token embeddings (the operator form) | 1 = compute them and keep a copy (drop iteration 0) | 2 = the
// images are those of the last embed-1 call with the patches of d_dropped zeroed: reuse the copy (embed_reuse_kernel)
static int vit_forward_impl(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, int32_t B, void* stream, int embed) {
    if (!e || !d_images) return PNP_ERR_ARG;
    if (!e->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch) return fail(e, PNP_ERR_ARG, "batch %d out of range (max %d)", B, e->c.max_batch);
    hipStream_t s = (hipStream_t)stream;
    const int D = e->D, N = e->N, M = B * N, F = D * e->c.vit_mlp_ratio, bf = e->bf;
    const int ldv = e->c.max_batch * e->Npad;
    if (embed == 2 && !(e->reuse.vit && e->reuse.images == d_images && e->reuse.B == B)) embed = 0;   // stale: recompute
    if (embed == 2 && d_dropped) {
        hipLaunchKernelGGL(embed_reuse_kernel, dim3(2048), dim3(256), 0, s, (const float*)e->x0, d_dropped, (const float*)e->patch_b,
                           (const float*)e->pos, e->x, M, N, D / 4);
        KCHK(e, launched());
    } else {
        KCHK(e, patchify(bf, d_images, d_dropped, e->patches, B, e->c.img_size, e->P, s));
        KCHK(e, cls_rows(e->cls, e->pos, e->x, B, N, D, s));
        {
            GemmArgs g = linear(e->patches, 768, e->patch_w, B * e->PP);
            g.bias = e->patch_b; g.resid = e->pos; g.ldr = D; g.out_f32 = e->x; g.ldo = D; g.row_div = e->PP;
            KCHK(e, egemm(e, g, s));
        }
        if (embed == 1) {
            HIPCHK(e, hipMemcpyAsync(e->x0, e->x, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
            e->reuse.images = d_images;
            e->reuse.B = B;
            e->reuse.vit = true;
        }
    }
    const float scale = 1.0f / sqrtf(64.f);
    // split-bf16 ("bf16x3"): every Linear of the block is a wide-kernel launch on (hi, lo) bf16 operand pairs -- three bf16 MFMA
    // passes per product, fp32-class result; LayerNorm, the attention kernel and the GELU epilogue hand the next GEMM its
    // operand already split (the handles' lo halves, null in the other modes)
    const int ln = bf | e->x3;                   // LayerNorm writes bf16 for the pair too
    for (int l = 0; l < e->c.vit_depth; l++) {
        const VitLayerW& w = e->vit[l];
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
    KCHK(e, layernorm(ln, e->x, e->vnorm_w, e->vnorm_b, e->c.vit_ln_eps, M, D, e->emb32, e->embT.hi, nullptr, nullptr, s, e->embT.lo));
    return pnp_cross_kv(e, B, stream);
}
extern "C" int pnp_vit_forward(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, int32_t B, void* stream) {
    if (e) e->reuse.vit = false;                 // the operator form writes e->x: x0 no longer describes what follows
    return vit_forward_impl(e, d_images, d_dropped, B, stream, 0);
}

// encoder_hidden_states -> key / value of every text layer's cross-attention (B/med.py:208-211): the reference
// projects image_embeds once per layer inside BertSelfAttention.forward; here all 12 layers are projected in four
// launches (natural + transposed layouts) right after the ViT, from the compute-type copy of image_embeds.
extern "C" int pnp_cross_kv(pnp_engine* e, int32_t B, void* stream) {
    if (!e) return PNP_ERR_ARG;
    if (!e->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
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
        GemmArgs g = linear(e->embT, D, e->ck_w, M);
        g.bias = e->ck_b; out(g, e->Knat, TL * H);
        KCHK(e, egemm(e, g, s));
    }
    {
        GemmArgs g = linear_t(e->embT, D, e->cv_w, M);
        g.bias = e->cv_b; g.bias_on_rows = 1; out(g, e->Vt, ldv); g.col_div = N; g.col_pad = e->Npad;
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
        GemmArgs g = linear(e->embT, D, e->cv_w, M, SL * H, nVn * H);
        g.bias = e->cv_b + (size_t)SL * H; g.out_t = e->Vnat; g.ldo_t = nVn * H;
        KCHK(e, egemm(e, g, s));
    }
    if (nKt > 0) {
        GemmArgs g = linear_t(e->embT, D, e->ck_w, M, (SL + 1) * H, nKt * H);
        g.bias = e->ck_b + (size_t)(SL + 1) * H; g.bias_on_rows = 1; g.out_t = e->Kt; g.ldo_t = ldv; g.col_div = N; g.col_pad = e->Npad;
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
    const TextLayerW& w = e->txt[i];
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
    if (!e->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch || L < 5 || L > e->c.max_text_len || ld < L)
        return fail(e, PNP_ERR_ARG, "text batch %d x %d (ld %d) out of range (max %d x %d)", B, L, ld, e->c.max_batch, e->c.max_text_len);
    hipStream_t s = (hipStream_t)stream;
    const int H = e->H, TL = e->TL, R = B * L;
    e->acts_text_only = false;
    if (reuse_prefix && !(e->reuse.text && e->reuse.ids == d_ids && e->reuse.mask == d_mask && e->reuse.B == B && e->reuse.L == L &&
                          e->reuse.ld == ld))
        reuse_prefix = false;                    // not the captions whose prefix is in place: compute it
    if (!reuse_prefix) {
        KCHK(e, text_embed(d_ids, ld, e->word, e->tpos, e->temb, B, L, H, e->c.enc_token_id, e->c.vocab, s));
        KCHK(e, layernorm(e->bf, e->temb, e->eln_w, e->eln_b, e->c.txt_ln_eps, R, H, e->h0, e->h0T, nullptr, nullptr, s));
    }
    for (int i = 0; i < TL; i++) {
        int r = text_layer(e, i, d_mask, ld, B, L, true, reuse_prefix && i == 0, s);
        if (r) return r;
    }
    KCHK(e, itm_head(e->ta[TL - 1].h_out, e->itm_w, e->itm_b, d_logits ? d_logits : e->logits_scratch, B, L, H, s));
    return PNP_OK;
}
extern "C" int pnp_text_forward_xattn(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t B,
                                      int32_t L, float* d_logits, void* stream) {
    if (e) e->reuse.text = false;
    return text_forward_impl(e, d_ids, d_mask, ld, B, L, d_logits, stream, false);
}

// BertModel.forward(mode="text") (B/med.py:565-568, 473): the text stack without its cross-attention sub-layers and without the
// [ENC] substitution, for T texts that need no image.  Runs in the multimodal pass's activation buffers (temb, h0, tmp, ctx_s, g and
// each layer's qkv / a_out / h_out with their compute-type copies; no stash is written), max_batch rows of text at a time, so what
// those buffers held for a GradCAM backward is gone: the reuse record, the kept layer and the backward are invalidated.  image_embeds
// and the cross K / V of the last pnp_vit_forward are not touched.
extern "C" int pnp_text_forward_text(pnp_engine* e, const int64_t* d_ids, const int64_t* d_mask, int32_t ld, int32_t T, int32_t L,
                                     float* d_hidden, void* stream) {
    if (!e || !d_ids || !d_mask) return PNP_ERR_ARG;
    if (T <= 0 || L < 2 || L > e->c.max_text_len || ld < L)
        return fail(e, PNP_ERR_ARG, "text batch %d x %d (ld %d) out of range (2 <= L <= %d, T > 0)", T, L, ld, e->c.max_text_len);
    if (!e->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    hipStream_t s = (hipStream_t)stream;
    const int H = e->H, TL = e->TL;
    e->reuse.text = false;
    e->grad_layer = -1;
    e->acts_text_only = true;
    for (int t0 = 0; t0 < T; t0 += e->c.max_batch) {
        const int B = T - t0 < e->c.max_batch ? T - t0 : e->c.max_batch, R = B * L;
        const int64_t* ids = d_ids + (size_t)t0 * ld;
        const int64_t* mask = d_mask + (size_t)t0 * ld;
        KCHK(e, text_embed(ids, ld, e->word, e->tpos, e->temb, B, L, H, -1, e->c.vocab, s));
        KCHK(e, layernorm(e->bf, e->temb, e->eln_w, e->eln_b, e->c.txt_ln_eps, R, H, e->h0, e->h0T, nullptr, nullptr, s));
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
    if (!e->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    const Weight& w = e->proj_w[which];
    if (!w.p || !e->proj_b[which])
        return fail(e, PNP_ERR_STATE, "missing weight %s.weight (the state dict held no %s.weight / .bias)", kProj[which], kProj[which]);
    hipStream_t s = (hipStream_t)stream;
    const int E = e->proj_E[which];
    if (e->bf) {
        // bf16 operands: rows are cast into xn (free between ViT forwards), as many at a time as it holds
        size_t cap = (size_t)e->c.max_batch * e->N * e->D / K;
        cap = cap < 16384 ? cap : 16384;           // (and few enough for the generic tiles: the wide bf16 kernel has no such epilogue)
        for (size_t r0 = 0; r0 < (size_t)rows; r0 += cap) {
            const int n = (int)((size_t)rows - r0 < cap ? (size_t)rows - r0 : cap);
            KCHK(e, cast_rows_bf16(d_x + r0 * row_stride, (int)row_stride, e->xn.hi, n, K, s));
            GemmArgs g = linear(e->xn.hi, K, w, n);
            g.bias = e->proj_b[which]; g.out_f32 = d_out + r0 * E; g.ldo = E;
            KCHK(e, egemm(e, g, s));
        }
    } else {
        GemmArgs g = linear(d_x, (int)row_stride, w, rows);
        g.bias = e->proj_b[which]; g.out_f32 = d_out; g.ldo = E;
        KCHK(e, egemm(e, g, s));
    }
    KCHK(e, l2_normalize_rows(d_out, rows, E, 1e-12f, s));
    return PNP_OK;
}

// sim = image_feat @ text_feat.t() (B/blip_image_text_matching.py:265).  Stateless.
extern "C" int pnp_itc_similarity(const float* d_img_feat, const float* d_txt_feat, int32_t B, int32_t T, int32_t E, float* d_sim,
                                  void* stream) {
    if (!d_img_feat || !d_txt_feat || !d_sim || B <= 0 || T <= 0 || E <= 0 || E % 4) return PNP_ERR_ARG;
    return itc_similarity(d_img_feat, d_txt_feat, d_sim, B, T, E, (hipStream_t)stream);
}

extern "C" int pnp_xattn_grad(pnp_engine* e, int32_t B, int32_t L, void* stream) {
    return pnp_xattn_grad_layer(e, B, L, e ? e->SL : 0, stream);
}

extern "C" int pnp_xattn_grad_layer(pnp_engine* e, int32_t B, int32_t L, int32_t layer, void* stream) {
    if (!e) return PNP_ERR_ARG;
    if (!e->finalized) return fail(e, PNP_ERR_STATE, "weights not finalized");
    if (B <= 0 || B > e->c.max_batch || L < 5 || L > e->c.max_text_len) return fail(e, PNP_ERR_ARG, "bad B/L");
    if (layer < e->SL || layer >= e->TL)
        return fail(e, PNP_ERR_ARG, "layer %d: cross-attention maps are kept for text layers %d..%d (stash_layer)", layer, e->SL, e->TL - 1);
    if (e->acts_text_only)
        return fail(e, PNP_ERR_STATE, "the text activations in place are those of pnp_text_forward_text: run pnp_text_forward_xattn first");
    hipStream_t s = (hipStream_t)stream;
    const int H = e->H, I = e->I, TL = e->TL, R = B * L, bf = e->bf, N = e->N, SL = e->SL;
    const int ldv = e->c.max_batch * e->Npad, nVn = TL - SL;
    e->grad_layer = layer;
    KCHK(e, itm_grad_seed(e->itm_w, e->dh, B, L, H, s));
    for (int i = TL - 1; i >= layer; i--) {
        const TextLayerW& w = e->txt[i];
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
                                float* d_out, float* d_logits, void* stream, int embed) {
    int r = vit_forward_impl(e, d_images, d_dropped, B, stream, embed);
    if (r) return r;
    // drop iterations 1..: same captions as iteration 0 (embed == 2 only comes from the drop loop; a stash layer of 0 keeps the
    // probabilities of layer 0's self-attention, which are in place as well)
    r = text_forward_impl(e, d_ids, d_mask, ld, B, L, d_logits, stream, embed == 2);
    if (r) return r;
    if (embed == 1) {                            // the prefix now in place belongs to these captions
        e->reuse.ids = d_ids; e->reuse.mask = d_mask; e->reuse.L = L; e->reuse.ld = ld;
        e->reuse.text = true;
    } else if (embed == 0) {
        e->reuse.text = false;
    }
    r = pnp_xattn_grad_layer(e, B, L, layer, stream);
    if (r) return r;
    return pnp_gradcam_gather(e, d_mask, ld, B, L, head, d_out, stream);
}
extern "C" int pnp_compute_gradcam_layer(pnp_engine* e, const float* d_images, const uint8_t* d_dropped, const int64_t* d_ids,
                                         const int64_t* d_mask, int32_t ld, int32_t B, int32_t L, int32_t layer, int32_t head,
                                         float* d_out, float* d_logits, void* stream) {
    return compute_gradcam_impl(e, d_images, d_dropped, d_ids, d_mask, ld, B, L, layer, head, d_out, d_logits, stream, 0);
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
        int r = compute_gradcam_impl(e, d_images, e->dropped, d_ids, d_mask, ld, B, L, layer, head, e->G, d_logits, stream, it == 0 ? 1 : 2);
        if (r) return r;
        r = pnp_drop_step(e, e->G, d_g0, d_agg, e->dropped, d_picks, it, B, L - 1, npick, drop_iter * npick, stream);
        if (r) return r;
    }
    return PNP_OK;
}

// =========================================================================================== introspection

extern "C" int pnp_get_buffer(pnp_engine* e, const char* name, void** d_ptr, size_t* bytes) {
    if (!e || !name || !d_ptr || !bytes) return PNP_ERR_ARG;
    const std::string n(name);
    const size_t B = e->c.max_batch, L = e->c.max_text_len;
    auto set = [&](void* ptr, size_t b) { *d_ptr = ptr; *bytes = b; return PNP_OK; };
    if (n == "image_embeds") return set(e->emb32, B * e->N * (size_t)e->D * 4);
    if (n == "image_embeds_t") return set(e->embT.hi, B * e->N * (size_t)e->D * e->esz);
    if (n == "x") return set(e->x, B * e->N * (size_t)e->D * 4);
    if (n == "P") return set(e->ta[e->grad_layer >= 0 ? e->grad_layer : e->SL].Pc, B * e->nh * L * (size_t)e->Nst * 4);
    if (n == "dP") return set(e->dPc, B * e->nh * L * (size_t)e->Nst * 4);
    if (n == "text_hidden") return set(e->ta[e->TL - 1].h_out, B * L * (size_t)e->H * 4);
    if (n == "h_last") return set(e->ta[e->TL - 1].h_out, B * L * (size_t)e->H * 4);
    if (n == "dropped") return set(e->dropped, B * (size_t)e->PP);
    if (n == "P_last" && e->ta[e->TL - 1].Pc) return set(e->ta[e->TL - 1].Pc, B * e->nh * L * (size_t)e->Nst * 4);
    if (n == "Kt" && e->Kt) return set(e->Kt, (size_t)(e->TL - e->SL - 1) * e->H * B * e->Npad * e->esz);
    if (n == "Vt") return set(e->Vt, (size_t)e->TL * e->H * B * e->Npad * e->esz);
    if (n == "dq_xattn") return set(e->dqc, B * L * (size_t)e->H * e->esz);
    if (n == "dctx_xattn") return set(e->dctxc, B * L * (size_t)e->H * e->esz);
    if (post_get_buffer(e, n, d_ptr, bytes)) return PNP_OK;
    return fail(e, PNP_ERR_ARG, "unknown buffer %s", name);
}

extern "C" size_t pnp_allocated_bytes(const pnp_engine* e) { return e ? e->alloc_bytes : 0; }

extern "C" int pnp_profile_enable(pnp_engine* e, int32_t on) {
    if (!e) return PNP_ERR_ARG;
    if (!e->gemm_prof) {
        if (!on) {
            e->crf_prof.on = false;
            return PNP_OK;
        }
        e->gemm_prof = new GemmProfile();
    }
    GemmProfile& pf = *e->gemm_prof;
    pf.on = on != 0;
    pf.period = on > 1 ? on : 1;
    pf.seq = 0;
    pf.used = 0;
    pf.launches = 0;
    pf.flops = 0;
    e->crf_prof.on = on != 0;
    e->crf_prof.used = 0;
    e->crf_prof.launches = 0;
    e->crf_prof.work = 0;
    e->crf_prof.lattice = 0;
    return PNP_OK;
}

extern "C" int pnp_profile_read_stage(pnp_engine* e, int32_t stage, int64_t* launches, double* work, double* ms) {
    if (!e || !launches || !work || !ms) return PNP_ERR_ARG;
    if (stage == 0) return pnp_profile_read(e, launches, work, ms);
    if (stage != 1 && stage != 2) return fail(e, PNP_ERR_ARG, "unknown profile stage %d", stage);
    auto& pf = e->crf_prof;
    double total = 0;
    for (int i = 0; i < pf.used; i++) {
        HIPCHK(e, hipEventSynchronize(pf.ev1[i]));
        float t = 0;
        HIPCHK(e, hipEventElapsedTime(&t, pf.ev0[i], pf.ev1[i]));
        total += t;
    }
    *launches = pf.launches;
    *work = stage == 1 ? pf.work : pf.lattice;
    *ms = total;
    return PNP_OK;
}

extern "C" int pnp_profile_read(pnp_engine* e, int64_t* launches, double* flops, double* ms) {
    if (!e || !launches || !flops || !ms) return PNP_ERR_ARG;
    if (!e->gemm_prof) {
        *launches = 0; *flops = 0; *ms = 0;
        return PNP_OK;
    }
    GemmProfile& pf = *e->gemm_prof;
    double total = 0;
    for (int i = 0; i < pf.used; i++) {
        HIPCHK(e, hipEventSynchronize(pf.ev1[i]));
        float t = 0;
        HIPCHK(e, hipEventElapsedTime(&t, pf.ev0[i], pf.ev1[i]));
        total += t;
    }
    *launches = pf.launches;
    *flops = pf.flops;
    *ms = total;
    return PNP_OK;
}

extern "C" int pnp_op_gemm(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                           int32_t K, const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo,
                           int32_t gelu, void* stream) {
    GemmArgs g = G_(d_A, lda, d_B, ldb, M, N, K);
    g.bias = d_bias; g.resid = d_resid; g.ldr = ldr; g.out_f32 = d_out_f32; g.ldo = ldo;
    g.mode = gelu ? GEMM_EPI_GELU : GEMM_EPI_LINEAR;
    return gemm_nt(bf, g, (hipStream_t)stream);
}

extern "C" int pnp_op_gemm_ex(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                              int32_t K, const float* d_bias, const float* d_resid, int32_t ldr, float* d_out_f32, int32_t ldo,
                              void* d_out_t, int32_t ldo_t, int32_t mode, void* stream) {
    GemmArgs g = G_(d_A, lda, d_B, ldb, M, N, K);
    g.bias = d_bias; g.resid = d_resid; g.ldr = ldr; g.out_f32 = d_out_f32; g.ldo = ldo; g.out_t = d_out_t; g.ldo_t = ldo_t;
    g.mode = mode ? GEMM_EPI_GELU : GEMM_EPI_LINEAR;
    return gemm_nt(bf, g, (hipStream_t)stream);
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
    GemmArgs g = G_(d_A_hi, lda, d_B_hi, ldb, M, N, K);
    g.A_lo = d_A_lo; g.B_lo = d_B_lo;
    g.bias = d_bias; g.bias_on_rows = bias_on_rows; g.resid = d_resid; g.ldr = ldr; g.out_f32 = d_out_f32; g.ldo = ldo;
    g.out_t = d_out_hi; g.out_lo = d_out_lo; g.ldo_t = ldo_t; g.col_div = col_div; g.col_pad = col_pad;
    g.mode = gelu ? GEMM_EPI_GELU : GEMM_EPI_LINEAR;
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
    GemmArgs g = G_(d_A, lda, d_B_hi, ldb, M, N, K);
    g.B_lo = d_B_lo; g.a_f32 = 1;
    g.bias = d_bias; g.resid = d_resid; g.ldr = ldr; g.out_f32 = d_out_f32; g.ldo = ldo;
    g.mode = mode; g.aux = d_aux; g.ld_aux = ld_aux;
    return gemm_nt(0, g, (hipStream_t)stream);
}

extern "C" int pnp_op_gemm_tokcols(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                                   int32_t K, const float* d_bias_rows, void* d_out_t, int32_t ldo_t, int32_t col_div,
                                   int32_t col_pad, void* stream) {
    if (!d_out_t || col_div < 0 || (col_div > 0 && col_pad < col_div)) return PNP_ERR_ARG;
    GemmArgs g = G_(d_A, lda, d_B, ldb, M, N, K);
    g.bias = d_bias_rows; g.bias_on_rows = 1; g.out_t = d_out_t; g.ldo_t = ldo_t; g.col_div = col_div; g.col_pad = col_pad;
    return gemm_nt(bf, g, (hipStream_t)stream);
}

extern "C" int pnp_op_gemm_args(int32_t bf, const void* d_A, int32_t lda, const void* d_B, int32_t ldb, int32_t M, int32_t N,
                                int32_t K, const float* d_bias, int32_t bias_on_rows, const float* d_resid, int32_t ldr,
                                float* d_out_f32, int32_t ldo, void* d_out_t, int32_t ldo_t, int32_t mode, float* d_aux,
                                int32_t ld_aux, int32_t row_div, int32_t col_div, int32_t col_pad, void* stream) {
    if (!d_A || !d_B || (!d_out_f32 && !d_out_t) || M <= 0 || N <= 0 || K <= 0 || lda < K || ldb < K) return PNP_ERR_ARG;
    if (mode < 0 || mode > 2 || (mode == GEMM_EPI_GELU_GRAD && !d_aux)) return PNP_ERR_ARG;
    if (row_div < 0 || col_div < 0 || (col_div > 0 && col_pad < col_div)) return PNP_ERR_ARG;
    GemmArgs g = G_(d_A, lda, d_B, ldb, M, N, K);
    g.bias = d_bias; g.bias_on_rows = bias_on_rows ? 1 : 0; g.resid = d_resid; g.ldr = ldr;
    g.out_f32 = d_out_f32; g.ldo = ldo; g.out_t = d_out_t; g.ldo_t = ldo_t;
    g.mode = mode; g.aux = d_aux; g.ld_aux = ld_aux; g.row_div = row_div; g.col_div = col_div; g.col_pad = col_pad;
    return gemm_nt(bf ? 1 : 0, g, (hipStream_t)stream);
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
