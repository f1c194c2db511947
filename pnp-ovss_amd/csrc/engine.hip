// The engine behind include/pnp_hip.h: owns weights + workspace on one MI355X.  This unit is its lifetime, the weight loader,
// introspection and profiling; the sequences of the hand-written kernels of this directory on the caller's stream are in
// model.hip (the model) and post.hip (post-processing), the entry points that need no engine in ops.hip, and the state all of
// them share is engine.h.  Host logic, but for one small layout kernel (transpose_cast_kernel_f32).
#include <cstring>

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

int new_weight(pnp_engine* e, int rows, int cols, bool pair, Weight* w) {
    *w = Weight{nullptr, rows, cols, pair ? 2 : (int)e->esz, pair};
    // a pair belongs to bf16x3, whose compute type is fp32
    return dalloc(e, *e->w, reinterpret_cast<char**>(&w->p), (size_t)rows * cols * e->esz);
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

// One tensor of the reference state dict and where it goes.  The three lists below (top level, ViT block, text layer) are the
// only place that names the keys and their sizes: pnp_create allocates the fp32 arrays from them, pnp_load_weight resolves a
// name through them, pnp_finalize_weights walks them to see that everything arrived.
struct Key {
    const char* name = "";
    float** slot = nullptr;    // the fp32 array it is copied into (biases, LN, embeddings); null: a GEMM weight, staged fp32 until finalize
    size_t total = 0;          // elements of that array: several keys may share one (the fused qkv_b, the layer-major ck_b / cv_b)
    size_t off = 0;            // this key's first element in it
    int rows = 1, cols = 0;
    int id = 0;                // GEMM weight: its index in finalize's array of staged pointers (the enums below)
};
Key small(const char* name, float** slot, int count, size_t off = 0, size_t total = 0) {
    return {name, slot, total ? total : (size_t)count, off, 1, count, 0};
}
Key gemm(const char* name, int id, int rows, int cols) { return {name, nullptr, 0, 0, rows, cols, id}; }

enum { W_PATCH };
enum { W_QKV, W_PROJ, W_FC1, W_FC2 };
enum { W_Q, W_K, W_V, W_SO, W_CQ, W_CK, W_CV, W_CO, W_I, W_O, W_MAX };

std::vector<Key> top_keys(Weights& w, const pnp_config& c) {
    const int D = c.vit_dim, H = c.txt_hidden, N = (c.img_size / 16) * (c.img_size / 16) + 1;
    return {small("visual_encoder.cls_token", &w.cls, D),
            small("visual_encoder.pos_embed", &w.pos, N * D),
            gemm("visual_encoder.patch_embed.proj.weight", W_PATCH, D, 768),
            small("visual_encoder.patch_embed.proj.bias", &w.patch_b, D),
            small("visual_encoder.norm.weight", &w.vnorm_w, D),
            small("visual_encoder.norm.bias", &w.vnorm_b, D),
            small("text_encoder.embeddings.word_embeddings.weight", &w.word, c.vocab * H),
            small("text_encoder.embeddings.position_embeddings.weight", &w.tpos, c.max_pos * H),
            small("text_encoder.embeddings.LayerNorm.weight", &w.eln_w, H),
            small("text_encoder.embeddings.LayerNorm.bias", &w.eln_b, H),
            small("itm_head.weight", &w.itm_w, 2 * H),
            small("itm_head.bias", &w.itm_b, 2)};
}
const char* const kVitPrefix = "visual_encoder.blocks.";
std::vector<Key> vit_keys(Weights& w, const pnp_config& c, int li) {
    VitLayerW& v = w.vit[li];
    const int D = c.vit_dim, F = D * c.vit_mlp_ratio;
    return {small("norm1.weight", &v.n1w, D),      small("norm1.bias", &v.n1b, D),
            gemm("attn.qkv.weight", W_QKV, 3 * D, D),   small("attn.qkv.bias", &v.qkv_b, 3 * D),
            gemm("attn.proj.weight", W_PROJ, D, D),     small("attn.proj.bias", &v.proj_b, D),
            small("norm2.weight", &v.n2w, D),      small("norm2.bias", &v.n2b, D),
            gemm("mlp.fc1.weight", W_FC1, F, D),        small("mlp.fc1.bias", &v.fc1_b, F),
            gemm("mlp.fc2.weight", W_FC2, D, F),        small("mlp.fc2.bias", &v.fc2_b, D)};
}
const char* const kTextPrefix = "text_encoder.encoder.layer.";
std::vector<Key> text_keys(Weights& w, const pnp_config& c, int li) {
    TextLayerW& t = w.txt[li];
    const int D = c.vit_dim, H = c.txt_hidden, I = c.txt_inter;
    const size_t l = (size_t)li * H, all = (size_t)c.txt_layers * H;   // this layer's part of the layer-major cross K / V biases, of all
    return {gemm("attention.self.query.weight", W_Q, H, H),            small("attention.self.query.bias", &t.qkv_b, H, 0, 3 * H),
            gemm("attention.self.key.weight", W_K, H, H),              small("attention.self.key.bias", &t.qkv_b, H, H, 3 * H),
            gemm("attention.self.value.weight", W_V, H, H),            small("attention.self.value.bias", &t.qkv_b, H, 2 * H, 3 * H),
            gemm("attention.output.dense.weight", W_SO, H, H),         small("attention.output.dense.bias", &t.so_b, H),
            small("attention.output.LayerNorm.weight", &t.sln_w, H),   small("attention.output.LayerNorm.bias", &t.sln_b, H),
            gemm("crossattention.self.query.weight", W_CQ, H, H),      small("crossattention.self.query.bias", &t.cq_b, H),
            gemm("crossattention.self.key.weight", W_CK, H, D),        small("crossattention.self.key.bias", &w.ck_b, H, l, all),
            gemm("crossattention.self.value.weight", W_CV, H, D),      small("crossattention.self.value.bias", &w.cv_b, H, l, all),
            gemm("crossattention.output.dense.weight", W_CO, H, H),    small("crossattention.output.dense.bias", &t.co_b, H),
            small("crossattention.output.LayerNorm.weight", &t.cln_w, H), small("crossattention.output.LayerNorm.bias", &t.cln_b, H),
            gemm("intermediate.dense.weight", W_I, I, H),              small("intermediate.dense.bias", &t.i_b, I),
            gemm("output.dense.weight", W_O, H, I),                    small("output.dense.bias", &t.o_b, H),
            small("output.LayerNorm.weight", &t.oln_w, H),             small("output.LayerNorm.bias", &t.oln_b, H)};
}

// pnp_create_shared: everything but the per-engine capacities (batch, text length), the stash layer (it has a rule of its own)
// and the [ENC] token id has to be the donor's.  pnp_config is int32 / float fields throughout, so it has no padding bytes.
static_assert(sizeof(pnp_config) == 20 * 4, "pnp_config: 20 four-byte fields");
bool same_model(pnp_config a, const pnp_config& b) {
    a.max_batch = b.max_batch; a.max_text_len = b.max_text_len; a.stash_layer = b.stash_layer; a.enc_token_id = b.enc_token_id;
    return memcmp(&a, &b, sizeof a) == 0;
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
    for (void* p : e->own.allocs) (void)hipFree(p);
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
    e->w = std::make_shared<Weights>();        // empty and unfinalized: what an engine refused below is left with
    e->w->device = cfg->device;
    if (donor) {
        if (!donor->w->finalized) return fail(e, PNP_ERR_STATE, "pnp_create_shared: the donor's weights are not finalized");
        if (!same_model(donor->c, *cfg))
            return fail(e, PNP_ERR_ARG, "pnp_create_shared: device, compute mode and model geometry must equal the donor's");
        if (cfg->stash_layer < donor->c.stash_layer)
            return fail(e, PNP_ERR_ARG, "pnp_create_shared: stash_layer %d below the donor's %d (its transposed backward weights "
                        "exist for layers >= %d only)", cfg->stash_layer, donor->c.stash_layer, donor->c.stash_layer);
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
    e->ta.resize(TL);
    if (e->x3) {                               // one 256 KB partial-tile slot + one flag per CU (64 MB): not shared between engines
        const int n_cu = device_cu_count();
        if (!n_cu || streamk_ws_create(&e->sk_ws, n_cu) != PNP_OK) return fail(e, PNP_ERR_HIP, "stream-K workspace allocation failed");
        e->own.bytes += (size_t)n_cu * 256 * 256 * 4;
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
        e->w = donor->w;
        e->shares_weights = true;
        return PNP_OK;
    }
    // the fp32 arrays the loader copies into (biases, LayerNorm, embeddings): one allocation per distinct array of the key lists
    e->w->vit.resize(c.vit_depth);
    e->w->txt.resize(TL);
    auto alloc_small = [e](const std::vector<Key>& keys) {
        for (const Key& k : keys)
            if (k.slot && !*k.slot) KCHK(e, dalloc(e, *e->w, k.slot, k.total));
        return (int)PNP_OK;
    };
    if (int r = alloc_small(top_keys(*e->w, c))) return r;
    for (int i = 0; i < c.vit_depth; i++)
        if (int r = alloc_small(vit_keys(*e->w, c, i))) return r;
    for (int i = 0; i < c.txt_layers; i++)
        if (int r = alloc_small(text_keys(*e->w, c, i))) return r;
    return PNP_OK;
}
extern "C" int pnp_create(const pnp_config* cfg, pnp_engine** out) { return create_impl(cfg, nullptr, out); }
extern "C" int pnp_create_shared(const pnp_config* cfg, pnp_engine* donor, pnp_engine** out) {
    if (!donor) return PNP_ERR_ARG;
    return create_impl(cfg, donor, out);
}

// =========================================================================================== weights

namespace {

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
    if (layer_of(kVitPrefix, e->c.vit_depth)) return find_key(vit_keys(*e->w, e->c, li), rest, s);
    if (layer_of(kTextPrefix, e->TL)) return find_key(text_keys(*e->w, e->c, li), rest, s);
    return find_key(top_keys(*e->w, e->c), n.c_str(), s);
}

// the optional ITC projections: 1 = `name` is one of the four tensors (staged like a GEMM weight until finalize), 0 = it is
// not, < 0 = its shape contradicts the model.  The embedding width E is the weight's first dimension.
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
    int& have = e->w->proj_E[which];
    if (have && have != (int)E)
        return fail(e, PNP_ERR_ARG, "%s: %lld rows, but the other tensor of this projection has %d", n.c_str(), (long long)E, have);
    have = (int)E;
    s.rows = (int)E;
    s.cols = bias ? 1 : K;
    return 1;
}

const float* staged(const Weights& w, const std::string& n) {   // null until a copy into the buffer has succeeded
    auto it = w.staged.find(n);
    return it == w.staged.end() || !w.loaded.count(n) ? nullptr : it->second;
}

// every tensor of a family must have arrived; st[id] <- the fp32 staging of its GEMM weights
int collect(pnp_engine* e, const std::string& prefix, const std::vector<Key>& keys, const float** st) {
    for (const Key& k : keys) {
        const std::string n = prefix + k.name;
        if (k.slot ? !e->w->loaded.count(n) : !(st[k.id] = staged(*e->w, n))) return fail(e, PNP_ERR_STATE, "missing weight %s", n.c_str());
    }
    return PNP_OK;
}

}  // namespace

extern "C" int pnp_load_weight(pnp_engine* e, const char* name, const float* data, const int64_t* shape, int32_t ndim,
                               int32_t on_device) {
    if (!e || !name || !data || !shape) return PNP_ERR_ARG;
    if (e->shares_weights) return fail(e, PNP_ERR_STATE, "this engine uses a donor's weights (pnp_create_shared)");
    Weights& w = *e->w;
    if (w.finalized) return fail(e, PNP_ERR_STATE, "weights already finalized");
    HIPCHK(e, hipSetDevice(e->c.device));
    Key s;
    const int pj = resolve_proj(e, name, shape, ndim, s);
    if (pj < 0) return pj;
    if (!pj && !resolve(e, name, s)) return PNP_OK;   // strict=False: not a tensor of this path
    size_t count = 1;
    for (int i = 0; i < ndim; i++) count *= (size_t)shape[i];
    if (count != (size_t)s.rows * s.cols) return fail(e, PNP_ERR_ARG, "%s: expected %d elements, got %zu", name, s.rows * s.cols, count);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    float* dst = s.slot ? *s.slot + s.off : nullptr;
    if (!s.slot) {                             // staged in a buffer that w owns from its allocation on; a second load of the name
        float*& b = w.staged[name];            // has the same count (the key's, or the projection's E) and overwrites it
        if (!b) HIPCHK(e, hipMalloc((void**)&b, count * 4));
        dst = b;
    }
    HIPCHK(e, hipMemcpy(dst, data, count * 4, kind));
    w.loaded.insert(name);
    return PNP_OK;
}

extern "C" int pnp_finalize_weights(pnp_engine* e) {
    if (!e) return PNP_ERR_ARG;
    Weights& w = *e->w;
    if (w.finalized) return PNP_OK;
    HIPCHK(e, hipSetDevice(e->c.device));
    const int D = e->D, H = e->H, I = e->I, TL = e->TL, F = D * e->c.vit_mlp_ratio;
    const float* st[W_MAX];
    if (int r = collect(e, "", top_keys(w, e->c), st)) return r;
    KCHK(e, make_weight(e, st[W_PATCH], D, 768, false, &w.patch_w));
    for (int i = 0; i < e->c.vit_depth; i++) {
        VitLayerW& v = w.vit[i];
        if (int r = collect(e, kVitPrefix + std::to_string(i) + ".", vit_keys(w, e->c, i), st)) return r;
        KCHK(e, make_weight(e, st[W_QKV], 3 * D, D, false, &v.qkv_w, e->x3));
        KCHK(e, make_weight(e, st[W_PROJ], D, D, false, &v.proj_w, e->x3));
        KCHK(e, make_weight(e, st[W_FC1], F, D, false, &v.fc1_w, e->x3));
        KCHK(e, make_weight(e, st[W_FC2], D, F, false, &v.fc2_w, e->x3));
    }
    // cross-attention K / V weights of all layers, layer-major, so one GEMM projects every layer
    KCHK(e, new_weight(e, TL * H, D, e->x3, &w.ck_w));
    KCHK(e, new_weight(e, TL * H, D, e->x3, &w.cv_w));
    for (int i = 0; i < TL; i++) {
        TextLayerW& t = w.txt[i];
        if (int r = collect(e, kTextPrefix + std::to_string(i) + ".", text_keys(w, e->c, i), st)) return r;
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
        KCHK(e, fill_weight(e, st[W_CK], w.ck_w, i * H, H));
        KCHK(e, fill_weight(e, st[W_CV], w.cv_w, i * H, H));
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
        const float *pw = staged(w, std::string(kProj[i]) + ".weight"), *bs = staged(w, std::string(kProj[i]) + ".bias");
        if (!pw || !bs) {
            w.proj_E[i] = 0;
            continue;
        }
        KCHK(e, make_weight(e, pw, w.proj_E[i], i == 0 ? D : H, false, &w.proj_w[i], e->x3));
        KCHK(e, dalloc(e, w, &w.proj_b[i], (size_t)w.proj_E[i]));
        HIPCHK(e, hipMemcpy(w.proj_b[i], bs, (size_t)w.proj_E[i] * 4, hipMemcpyDeviceToDevice));
    }
    HIPCHK(e, hipDeviceSynchronize());
    w.drop_staging();
    w.finalized = true;
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

// (a sharing engine holds no weight bytes of its own: they are counted once, by the engine that loaded them)
extern "C" size_t pnp_allocated_bytes(const pnp_engine* e) { return e ? e->own.bytes + (e->shares_weights ? 0 : e->w->bytes) : 0; }

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
