// Internal to csrc/ (not installed, never included from include/): the engine's state and the few helpers its translation
// units share -- engine.hip (lifetime, weights, introspection), model.hip (the model sequence and the drop loop), ops.hip (operator
// shims and the entry points without engine state) and post.hip (post-processing).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pnp_hip.h"
#include "common.h"
#include "crf_solver.h"
#include "kernels.h"

namespace pnp {

// A GEMM weight [rows, cols] in the engine's compute mode.  bf16x3 keeps the wide Linears' weights as a (hi | lo) bf16 pair in the
// bytes of the fp32 copy: the hi array, then the lo array.  Only this type and new_weight / fill_weight know it.
struct Weight {
    void* p = nullptr;
    int rows = 0, cols = 0;
    int esz = 0;               // bytes per stored element
    bool pair = false;
    void* hi(int r0 = 0) const { return (char*)p + (size_t)r0 * cols * esz; }      // row r0 on: a layer of the layer-major ck_w / cv_w
    void* lo(int r0 = 0) const { return pair ? (char*)p + ((size_t)rows + r0) * cols * esz : nullptr; }
};

// An activation buffer of the ViT side: one array of the compute type, or in bf16x3 a (hi, lo) bf16 pair whose lo array starts
// at the buffer's row capacity, whatever batch is in flight (alloc_act)
struct Act {
    void* hi = nullptr;
    void* lo = nullptr;        // null outside bf16x3
};

struct TextLayerW {
    // forward (T = compute dtype)
    Weight qkv_w, so_w, cq_w, co_w, i_w, o_w;
    float *qkv_b = nullptr, *so_b = nullptr, *sln_w = nullptr, *sln_b = nullptr, *cq_b = nullptr, *co_b = nullptr,
          *cln_w = nullptr, *cln_b = nullptr, *i_b = nullptr, *o_b = nullptr, *oln_w = nullptr, *oln_b = nullptr;
    // backward (transposed copies, layers >= stash_layer)
    Weight o_wT, i_wT, co_wT, cq_wT, so_wT, qkv_wT;
};

struct TextLayerA {
    void* qkv = nullptr;       // T [R,3H]
    float* Ps = nullptr;       // [B,nh,L,L]
    float *a_hat = nullptr, *a_rstd = nullptr, *a_out = nullptr;
    void* a_outT = nullptr;
    void* qc = nullptr;        // T [R,H]
    float* Pc = nullptr;       // [B,nh,L,Nst]  (layers >= stash only)
    float *c_hat = nullptr, *c_rstd = nullptr, *c_out = nullptr;
    void* c_outT = nullptr;
    float* u = nullptr;        // [R,I]
    float *o_hat = nullptr, *o_rstd = nullptr, *h_out = nullptr;
    void* h_outT = nullptr;
};

struct VitLayerW {
    float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr, *qkv_b = nullptr, *proj_b = nullptr, *fc1_b = nullptr,
          *fc2_b = nullptr;
    Weight qkv_w, proj_w, fc1_w, fc2_w;
};

// A list of device allocations and what they add up to: the engine's own (activations, workspace) or a Weights'
struct Allocs {
    std::vector<void*> allocs;
    size_t bytes = 0;
};

// Everything pnp_load_weight / pnp_finalize_weights produce (converted GEMM weights, biases, LayerNorm parameters, embeddings)
// and the device memory behind it: read-only once finalized, so several engines of a process may use one copy
// (pnp_create_shared); freed with the last engine that holds it.
struct Weights : Allocs {
    int device = 0;
    bool finalized = false;
    // the loader's state, empty once finalized: fp32 device staging of the GEMM weights by tensor name, names that arrived
    std::map<std::string, float*> staged;
    std::set<std::string> loaded;

    float *cls = nullptr, *pos = nullptr, *patch_b = nullptr, *vnorm_w = nullptr, *vnorm_b = nullptr;
    Weight patch_w;
    std::vector<VitLayerW> vit;
    float *word = nullptr, *tpos = nullptr, *eln_w = nullptr, *eln_b = nullptr, *itm_w = nullptr, *itm_b = nullptr;
    std::vector<TextLayerW> txt;
    // optional ITC projections, [0] vision_proj (D -> E), [1] text_proj (H -> E) (B/blip_image_text_matching.py:54-55): present when
    // the state dict carried weight and bias; E is read from the weight's first dimension
    Weight proj_w[2];
    float* proj_b[2] = {nullptr, nullptr};
    int proj_E[2] = {0, 0};
    Weight ck_w, cv_w;                         // cross K / V weights of all layers: [TL*H, D]
    float *ck_b = nullptr, *cv_b = nullptr;    // [TL*H]

    void drop_staging() {
        for (auto& s : staged) (void)hipFree(s.second);
        staged.clear();
        loaded.clear();
    }
    Weights() = default;
    Weights(const Weights&) = delete;
    ~Weights() {
        (void)hipSetDevice(device);
        drop_staging();
        for (void* p : allocs) (void)hipFree(p);
    }
};

}  // namespace pnp

struct pnp_engine {
    pnp_config c{};
    std::shared_ptr<pnp::Weights> w;           // never null; with shares_weights, a donor's (pnp_create_shared)
    bool shares_weights = false;
    int bf = 0;                // 1: bf16 storage / bf16 MFMA everywhere
    int x3 = 0;                // 1: split-bf16 ("bf16x3") ViT Linears + cross K/V projections, everything else as fp32 mode
    size_t esz = 4;
    int P = 0, PP = 0, N = 0, Npad = 0, D = 0, H = 0, I = 0, TL = 0, nh = 0, Nst = 0, SL = 0;
    char err[512] = {0};
    pnp::Allocs own;           // what this engine alone holds: activations and workspace

    // ---- activations
    int ldq = 0;               // row stride (elements) of the fused q|k|v buffer
    float* x0 = nullptr;       // [M, D] token embeddings of drop iteration 0 (patch embed + pos, cls row): later iterations reuse them
    void *patches = nullptr, *vt = nullptr;
    pnp::Act xn, qk, ctx, h1, embT;
    float *x = nullptr, *emb32 = nullptr;
    void *Knat = nullptr, *Vnat = nullptr, *Kt = nullptr, *Vt = nullptr;
    std::vector<pnp::TextLayerA> ta;
    float *temb = nullptr, *h0 = nullptr, *tmp = nullptr;
    void *h0T = nullptr, *ctx_s = nullptr, *ctx_c = nullptr, *g = nullptr;
    // backward
    float *dh = nullptr, *d_pre = nullptr, *dc = nullptr, *d_cpre = nullptr, *da = nullptr, *d_apre = nullptr,
          *dctx_s = nullptr, *dS = nullptr, *dPc = nullptr;
    void *d_preT = nullptr, *dg = nullptr, *d_cpreT = nullptr, *dctxc = nullptr, *dqc = nullptr, *d_apreT = nullptr,
         *dqkv = nullptr;
    int grad_layer = -1;       // text layer whose dL/dP the dPc buffer currently holds (-1: none)
    bool acts_text_only = false;   // the text activations in place are those of pnp_text_forward_text (no cross-attention: no backward)
    // drop loop
    float* G = nullptr;
    uint8_t* dropped = nullptr;
    float* logits_scratch = nullptr;

    // ---- post-process state (post.hip)
    struct Post {
        bool reserved = false, prepared = false, has_crf = false;
        // -- fixed by pnp_post_reserve: bounds, capacities (elements) and the device arrays
        int groups_cap = 1;                   // 2: the CRF arrays were sized for the paired (two-group) run
        int maxB = 0, maxK = 0, maxKp = 0, max_pix_img = 0, chunk = 0;
        int64_t max_total_pix = 0;
        int lut_cap = 0, cls_cap = 0, tok_cap = 0, wts_cap = 0;
        int32_t *d_img_cls_off = nullptr, *d_cls_off = nullptr, *d_tok_idx = nullptr, *d_cls_div = nullptr, *d_lut = nullptr;
        size_t* d_label_off = nullptr;
        double* d_wts = nullptr;
        int32_t* d_wt_off = nullptr;
        float *merged = nullptr, *thr = nullptr, *maps = nullptr, *maps2 = nullptr, *maps3 = nullptr, *stats = nullptr;
        pnp::CrfWorkspace crf;                // the DenseCRF arrays, sized for groups_cap groups per row and chunks of `chunk` images
        // -- the batch of the last pnp_post_prepare
        int B = 0, Cmax = 0, Kmax = 0, maxHW = 0, maxH = 0, maxW = 0, max_radius = 0;
        int lut_stride = 0;
        std::vector<pnp::PostDesc> desc[2];   // host copies of the two layouts; [0] is the batch's geometry for every host loop
        // the prepared batch in its two layouts: [0] one channel group per row, [1] the paired run's two (1-drop | N-drop)
        pnp::CrfSpan view[2]{};               // (d_desc and groups are fixed by reserve, kp_max is the batch's)
        // host staging of the per-batch tables: lives in the engine until the next prepare (pageable memory: the runtime copies
        // it into its own staging buffer at enqueue time, so rewriting it on the next call is safe without a synchronisation)
        std::vector<size_t> h_label_off;      // [B + 1] first pixel of every image; [B]: the pixels of the batch
        std::vector<int32_t> h_wt_off;
        std::vector<double> h_wts;
        const uint8_t* d_rgb = nullptr;
        const float* d_gt = nullptr;
        bool maps_in_2 = false;               // where the current maps live after blur
    } post;

    pnp::GemmProfile* gemm_prof = nullptr;     // live timing ring of this engine's dense GEMM launches (allocated on first enable)
    pnp::StreamKWs sk_ws;                      // partial tiles + flags of the in-launch reductions (split-bf16 mode: gemm_x3.hip)
    // live timing of one pipeline stage (bench.py's hbm roofline record for the DenseCRF mean-field): event pairs
    // on the launch stream around the stage, algorithmic bytes summed beside them
    struct StageProfile {
        bool on = false;
        std::vector<hipEvent_t> ev0, ev1;
        int used = 0;
        long long launches = 0;
        double work = 0;                       // SURVEY.md 8d bytes of the bracketed iterations
        double lattice = 0;                    // lattice-blur term of the same brackets (reported separately)
    } crf_prof;
};

namespace pnp {

inline int fail(pnp_engine* e, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e->err, sizeof(e->err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(e, call)                                                                      \
    do {                                                                                     \
        hipError_t _s = (call);                                                              \
        if (_s != hipSuccess) return fail(e, PNP_ERR_HIP, "%s: %s", #call, hipGetErrorString(_s)); \
    } while (0)
#define KCHK(e, call)                                                         \
    do {                                                                      \
        int _r = (call);                                                      \
        if (_r != PNP_OK) return fail(e, _r, "%s failed (%d): %s", #call, _r, hipGetErrorString(hipGetLastError())); \
    } while (0)

// the one allocation routine: `count` elements of T that `owner` frees (e->own, or *e->w for a weight); errors go to e
template <typename T>
inline int dalloc(pnp_engine* e, Allocs& owner, T** out, size_t count, bool zero = false) {
    void* p = nullptr;
    const size_t bytes = (count * sizeof(T) + 255) / 256 * 256;
    if (hipMalloc(&p, bytes ? bytes : 256) != hipSuccess) return fail(e, PNP_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    owner.allocs.push_back(p);
    owner.bytes += bytes;
    if (zero && hipMemset(p, 0, bytes ? bytes : 256) != hipSuccess) return fail(e, PNP_ERR_HIP, "hipMemset failed");
    *out = reinterpret_cast<T*>(p);
    return PNP_OK;
}
template <typename T>
inline int dalloc(pnp_engine* e, T** out, size_t count, bool zero = false) { return dalloc(e, e->own, out, count, zero); }
inline int dalloc_t(pnp_engine* e, void** out, size_t count, bool zero = false) {   // `count` elements of the compute type
    char* p = nullptr;
    int r = dalloc(e, &p, count * e->esz, zero);
    *out = p;
    return r;
}
// a raw kernel launch: KCHK(e, launched()) right behind it
inline int launched() { return hipPeekAtLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP; }   // (KCHK reads and clears the error)

// state-dict names of the optional ITC projections, [0] / [1] as in Weights::proj_w
inline const char* const kProj[2] = {"vision_proj", "text_proj"};

inline GemmArgs G_(const void* A, int lda, const void* B, int ldb, int M, int N, int K) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    return g;
}

// The launch of a Linear in the engine's mode, y[M, n] = a[M, K] . w[r0 .. r0 + n, K]^T (n = 0: the whole weight); the caller
// adds the epilogue.  A pair weight (bf16x3) meets either a pair activation, or one fp32 array whose rows the kernel splits
// (a_f32: the text side, gemm_nt_small_x3_kernel).
inline GemmArgs linear(const void* a, int lda, const Weight& w, int M, int r0 = 0, int n = 0) {
    GemmArgs g = G_(a, lda, w.hi(r0), w.cols, M, n ? n : w.rows, w.cols);
    g.B_lo = w.lo(r0);
    g.a_f32 = w.pair;
    return g;
}
inline GemmArgs linear(const Act& a, int lda, const Weight& w, int M, int r0 = 0, int n = 0) {
    GemmArgs g = linear(a.hi, lda, w, M, r0, n);
    g.A_lo = a.lo;
    g.a_f32 = w.pair && !a.lo;
    return g;
}
// the same product written feature-major, y^T[n, M] = w . a^T: the operands change places
inline GemmArgs linear_t(const Act& a, int lda, const Weight& w, int M, int r0 = 0, int n = 0) {
    GemmArgs g = linear(a, lda, w, M, r0, n);
    std::swap(g.A, g.B); std::swap(g.A_lo, g.B_lo); std::swap(g.lda, g.ldb); std::swap(g.M, g.N);
    return g;
}

// every GEMM of an engine goes through here: the launch is timed into the engine's own ring when profiling is on.  gemm_nt
// takes the bf16 kernels by itself when an operand is a pair
inline int egemm(pnp_engine* e, GemmArgs g, hipStream_t s) {
    g.prof = e->gemm_prof;
    g.sk = e->sk_ws.part ? &e->sk_ws : nullptr;
    return gemm_nt(e->bf, g, s);
}

// post.hip's share of pnp_get_buffer: the post-process arrays by name (false: not one of them, or nothing reserved yet)
bool post_get_buffer(pnp_engine* e, const std::string& name, void** d_ptr, size_t* bytes);

}  // namespace pnp
