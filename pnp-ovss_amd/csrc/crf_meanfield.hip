// The forward mean-field of the DenseCRF on the lattices of crf_lattice.hip (the algorithm and its contract: that file's
// header): splat, lattice blurs and the three update kernels, with their launchers.  Shared helpers and the XCD work
// distribution of these kernels: crf_device.h; the pieces the update kernels are put together from: crf_tile.h.
#include "crf_tile.h"

namespace pnp {

// ------------------------------------------------------------------------------------------
// Mean-field iteration kernels.  Values / Q / unary rows are padded to Kp = 4*ceil(K/4) floats so
// every access is one 16-byte vector per lane (pad channels carry zeros and are never read back as
// labels).  Arithmetic per channel is exactly the scalar sequence of the oracle.

// splat: val[id] = sum over the lattice point's contributors (ascending pixel) of bary * (Q * norm).
// LPP lanes share one lattice point (one 16-byte channel chunk each).  The contributor records of the point -- (pixel, bary,
// norm) triples stored in list order by the lattice build -- are loaded LPP at a time, one 16-byte record per lane (one
// coalesced load instead of a dependent index -> weight -> norm chain per contributor), handed round the group with lane
// shuffles, and up to eight Q-row gathers are in flight per lane before the ordered accumulation.  The kernel is bound by
// memory latency x occupancy, not by bytes, so the chain segment -> records -> rows is software-pipelined over the
// grid-stride loop: while the rows of point t are gathered, the records of point t+1 and the segment of point t+2 are
// already in flight (one exposed latency per point instead of three).  Per-channel arithmetic and order are those of the
// sequential CPU algorithm (oracle/densecrf_ref.c::lattice_compute).  WHICH only names the instantiation in profiles.
template <int LPP, int WHICH, bool MULTI>
__global__ __launch_bounds__(256) void crf_splat_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs,
                                                        const float* __restrict__ Q, float* __restrict__ val, int img0, int nimg) {
    constexpr int PPB = 256 / LPP;                       // lattice points per workgroup pass
    constexpr int G = 8;                                 // row gathers in flight per lane
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int c0 = threadIdx.x & (LPP - 1), pl = threadIdx.x / LPP;
    const int stride = bpx * PPB;
    const CrfEntry none = {0u, 0.f, 0.f, 0u};
    int b, part, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part, parts); wi++) {
        const PostDesc im = imgs[b];
        const int K4 = im.Kp >> 2;
        const int lo = L.idbase[b], hi = L.idbase[b + 1];
        // rows are addressed as base + 32-bit byte offset (an image's Q block is < 4 GB; pixels per image < 2^24)
        const char* const Qb = reinterpret_cast<const char*>(Q + im.qoff);
        const uint32_t rowb = (uint32_t)K4 * 16u;
        f32x4* V4 = reinterpret_cast<f32x4*>(val + im.voff[L.which]);
        const int r0 = (int)((long)(hi - lo) * part / parts), r1 = (int)((long)(hi - lo) * (part + 1) / parts);
        int idl = r0 + slot * PPB + pl;
        // pipeline prologue: segment of points t and t+1, first record chunk of point t
        int e0 = 0, e1 = 0, e0n = 0, e1n = 0;
        if (idl < r1) {
            e0 = L.seg_lo[lo + idl];
            e1 = L.seg_hi[lo + idl];
        }
        if (idl + stride < r1) {
            e0n = L.seg_lo[lo + idl + stride];
            e1n = L.seg_hi[lo + idl + stride];
        }
        CrfEntry first = none;
        if (c0 < e1 - e0) first = ld_entry(L.ent + e0 + c0);
        f32x4 prev_acc = {0.f, 0.f, 0.f, 0.f};
        size_t prev_at = 0;
        bool have_prev = false;
        // up to G row gathers of a record chunk (records j0 .. of `mine`, n valid), then their ordered accumulation
        auto gather = [&](const CrfEntry& mine, int j0, int n, uint32_t cofs, f32x4* in) {
#pragma unroll
            for (int j = 0; j < G; j++) {
                if (j == 0 || j0 + j < n) {
                    const uint32_t px = (uint32_t)__shfl((int)mine.pixel, j0 + j, LPP) - (uint32_t)im.pix0;
                    in[j] = *reinterpret_cast<const f32x4*>(Qb + (__umul24(px, rowb) + cofs));
                }
            }
        };
        auto accumulate = [&](const CrfEntry& mine, int j0, int n, const f32x4* in, f32x4& acc) {
#pragma unroll
            for (int j = 0; j < G; j++) {
                if (j == 0 || j0 + j < n) {
                    const float w = __shfl(mine.w, j0 + j, LPP), nr = __shfl(mine.nr, j0 + j, LPP);
#pragma unroll
                    for (int i = 0; i < 4; i++) acc[i] = __fadd_rn(acc[i], __fmul_rn(w, __fmul_rn(in[j][i], nr)));
                }
            }
        };
        for (; idl < r1; idl += stride) {
            // segment of point t+2 and first records of point t+1 are requested right behind the first gather group of point
            // t (straight-line code, nothing pending in front of it), so the three latencies overlap: the compiler's wait in
            // front of the accumulation covers them all
            int e0nn = 0, e1nn = 0;
            CrfEntry firstn = none;
            auto prefetch = [&]() {
                if (idl + 2 * stride < r1) {
                    e0nn = L.seg_lo[lo + idl + 2 * stride];
                    e1nn = L.seg_hi[lo + idl + 2 * stride];
                }
                if (c0 < e1n - e0n) firstn = ld_entry(L.ent + e0n + c0);
            };
            if (MULTI) prefetch();
            // MULTI: rows wider than LPP chunks take several passes over the point's records (cb loop; the prefetch then sits
            // in front of the loop and is waited for first); the common case is one straight-line pass
            for (int cb = 0; cb < (MULTI ? K4 : 1); cb += LPP) {
                const uint32_t cofs = (uint32_t)(cb + c0 < K4 ? cb + c0 : K4 - 1) * 16u;   // lanes past the row keep a valid chunk (they carry records)
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                f32x4 in[G];
                int n = e1 - e0 < LPP ? e1 - e0 : LPP;                    // (the same in all lanes of the group)
                gather(first, 0, n, cofs, in);
                if (!MULTI) {
                    prefetch();
                    if (have_prev) st_stream(V4 + prev_at, prev_acc);     // the previous point's row, stored under this point's gathers
                    asm volatile("" ::: "memory");                        // (keeps every request above in front of the wait below)
                }
                accumulate(first, 0, n, in, acc);
                for (int j0 = G; j0 < n; j0 += G) {
                    gather(first, j0, n, cofs, in);
                    accumulate(first, j0, n, in, acc);
                }
                for (int eb = e0 + LPP; eb < e1; eb += LPP) {
                    n = e1 - eb < LPP ? e1 - eb : LPP;
                    const CrfEntry mine = c0 < n ? ld_entry(L.ent + eb + c0) : none;
                    for (int j0 = 0; j0 < n; j0 += G) {
                        gather(mine, j0, n, cofs, in);
                        accumulate(mine, j0, n, in, acc);
                    }
                }
                if (MULTI) {
                    if (cb + c0 < K4) st_stream(V4 + (size_t)idl * K4 + cb + c0, acc);
                } else {                                                  // stored one point later (a store waited for at the loop
                    prev_acc = acc;                                       // head would expose its acknowledge latency)
                    prev_at = (size_t)idl * K4 + c0;
                    have_prev = c0 < K4;
                }
            }
            e0 = e0n; e1 = e1n; e0n = e0nn; e1n = e1nn;
            first = firstn;
        }
        if (have_prev) st_stream(V4 + prev_at, prev_acc);
    }
}

// one axis of the lattice blur: new = old + 0.5 * (n1 + n2), absent neighbours contribute 0.
// Work items are (lattice point, 16-byte channel chunk) pairs in linear order, so a wave touches 1 KB of
// consecutive value bytes whatever Kp is (no idle lanes at Kp = 24), and every thread keeps two items -- six
// independent value gathers behind four index loads -- in flight.  (The same item order made the splat
// slower: its lanes then diverge on the contributor counts of more points per wave.)
__global__ __launch_bounds__(256) void crf_blur4_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs,
                                                        const float* __restrict__ src, float* __restrict__ dst, int axis,
                                                        int img0, int nimg) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int* n1 = L.n1 + (size_t)axis * L.cap;
    const int* n2 = L.n2 + (size_t)axis * L.cap;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int b, part, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part, parts); wi++) {
        // The descriptor's fields are read where they are needed (scalar loads).  A by-value copy indexed with L.which is kept
        // per lane in LDS (18 KB per workgroup), and what is derived from it -- K4, the bases, the item range -- then sits in
        // vector registers although it is the same in all lanes: 41 -> 29 registers here, 72 -> 60 in crf_blur4x2_kernel.
        const PostDesc& im = imgs[b];
        const int K4 = im.Kp >> 2;
        const int lo = L.idbase[b], hi = L.idbase[b + 1];
        const size_t voff = L.which ? im.voff[1] : im.voff[0];
        const f32x4* S4 = reinterpret_cast<const f32x4*>(src + voff);
        f32x4* D4 = reinterpret_cast<f32x4*>(dst + voff);
        const int first = (int)((long)(hi - lo) * part / parts) * K4;
        const int nitem = (int)((long)(hi - lo) * (part + 1) / parts) * K4, stride = bpx * 256;
        for (int it0 = first + slot * 256 + threadIdx.x; it0 < nitem; it0 += 2 * stride) {
            const int it1 = it0 + stride;
            const bool two = it1 < nitem;
            const int p0 = it0 / K4, p1 = two ? it1 / K4 : p0;
            const int a0 = n1[lo + p0], d0 = n2[lo + p0], a1 = n1[lo + p1], d1 = n2[lo + p1];
            const int c0 = it0 - p0 * K4, c1 = (two ? it1 : it0) - p1 * K4;
            const f32x4 va0 = a0 >= 0 ? S4[(size_t)(a0 - lo) * K4 + c0] : zero;
            const f32x4 vd0 = d0 >= 0 ? S4[(size_t)(d0 - lo) * K4 + c0] : zero;
            const f32x4 old0 = S4[it0];
            const f32x4 va1 = a1 >= 0 ? S4[(size_t)(a1 - lo) * K4 + c1] : zero;
            const f32x4 vd1 = d1 >= 0 ? S4[(size_t)(d1 - lo) * K4 + c1] : zero;
            const f32x4 old1 = S4[two ? it1 : it0];
            f32x4 o0, o1;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                o0[i] = crf_axis(old0[i], va0[i], vd0[i]);
                o1[i] = crf_axis(old1[i], va1[i], vd1[i]);
            }
            D4[it0] = o0;
            if (two) D4[it1] = o1;
        }
    }
}

// Two consecutive axes of the lattice blur in one pass: out = B_{axis+1}(B_axis(src)).  The intermediate B_axis(src) is
// recomputed at the point and at its two axis+1 neighbours with exactly the single-axis arithmetic (each rounded to fp32 as
// the stored intermediate would be), so the result equals two crf_blur4 passes bit for bit while the value array is
// streamed from / to HBM once instead of twice; the 8 neighbour rows of a point sit close to it in the spatial numbering
// and are served by L2.  Same (point, 16-byte chunk) item order and XCD schedule as crf_blur4.
__device__ __forceinline__ f32x4 crf_blur1(const f32x4& old, const f32x4& va, const f32x4& vd) {
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = crf_axis(old[i], va[i], vd[i]);
    return o;
}
// The eight neighbour ids of a point for the axis pair (2p, 2p+1) come from one 32-byte record (CrfNbr8, image-local ids,
// built once per lattice) instead of two dependent rounds of index loads; rows are addressed with 32-bit byte offsets; the
// record of the thread's next item is requested behind the row gathers of the current one and the previous result is
// stored there too, so an item exposes one memory latency (the kernel is bound by latency x occupancy and by the 64 B/clk
// of the CU's vector memory path -- nine rows in, one out -- not by HBM bytes).  60 registers: eight waves per SIMD (seven at
// the 72 of the by-value descriptor: 300 -> 281 us per launch on the headline batch, profiles/crf_occupancy.txt).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8)))
void crf_blur4x2_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs,
                                                          const float* __restrict__ src, float* __restrict__ dst, int pair,
                                                          int img0, int nimg) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int b, part, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part, parts); wi++) {
        const PostDesc& im = imgs[b];                                   // (fields read one by one: see crf_blur4_kernel)
        const int K4 = im.Kp >> 2;
        const int lo = L.idbase[b], hi = L.idbase[b + 1];
        const size_t voff = L.which ? im.voff[1] : im.voff[0];
        const char* const Sb = reinterpret_cast<const char*>(src + voff);
        f32x4* const D4 = reinterpret_cast<f32x4*>(dst + voff);
        const CrfNbr8* const T = L.nbr8 + (size_t)pair * L.cap + lo;
        const uint32_t rowb = (uint32_t)K4 * 16u;
        const int first = (int)((long)(hi - lo) * part / parts) * K4;
        const int nitem = (int)((long)(hi - lo) * (part + 1) / parts) * K4, stride = bpx * 256;
        const int sq = stride / K4, sr = stride - sq * K4;              // item -> (point, chunk) advances without a division
        int it = first + slot * 256 + threadIdx.x;
        int p = it / K4, c = it - p * K4;
        CrfNbr8 t = {-1, -1, -1, -1, -1, -1, -1, -1};
        if (it < nitem) t = T[p];
        f32x4 prev = zero;
        int prev_it = -1;
        for (; it < nitem; it += stride) {
            const uint32_t cofs = (uint32_t)c * 16u;
#define PNP_ROW(x) ((x) >= 0 ? *reinterpret_cast<const f32x4*>(Sb + (__umul24((uint32_t)(x), rowb) + cofs)) : zero)
            const f32x4 r_i = *reinterpret_cast<const f32x4*>(Sb + (__umul24((uint32_t)p, rowb) + cofs));
            const f32x4 r_ia = PNP_ROW(t.ia), r_id = PNP_ROW(t.id);
            const f32x4 r_a = PNP_ROW(t.pa), r_aa = PNP_ROW(t.aa), r_ad = PNP_ROW(t.ad);
            const f32x4 r_d = PNP_ROW(t.pd), r_da = PNP_ROW(t.da), r_dd = PNP_ROW(t.dd);
#undef PNP_ROW
            // next item's neighbour record and the previous item's result go out behind the gathers
            int pn = p + sq, cn = c + sr;
            if (cn >= K4) {
                cn -= K4;
                pn++;
            }
            CrfNbr8 tn = {-1, -1, -1, -1, -1, -1, -1, -1};
            if (it + stride < nitem) tn = T[pn];
            if (prev_it >= 0) st_stream(D4 + prev_it, prev);   // (streamed: the next pass reads it back from beyond L2 either way)
            asm volatile("" ::: "memory");
            const f32x4 m_i = crf_blur1(r_i, r_ia, r_id);
            const f32x4 m_a = t.pa >= 0 ? crf_blur1(r_a, r_aa, r_ad) : zero;
            const f32x4 m_d = t.pd >= 0 ? crf_blur1(r_d, r_da, r_dd) : zero;
            prev = crf_blur1(m_i, m_a, m_d);
            prev_it = it;
            t = tn;
            p = pn;
            c = cn;
        }
        if (prev_it >= 0) st_stream(D4 + prev_it, prev);
    }
}

// Fused tail of a mean-field iteration for a tile of up to 256 pixels:
//   t = -U - (-w_g * norm_g * slice_g) - (-w_b * norm_b * slice_b)   (both lattices already blurred)
//   Q = exp(t - max_k t) / sum_k          (per pixel, staged through LDS so global I/O stays 16-B wide)
// pairwise == 0: Q = softmax(-U) (the initial marginals).
// A tile is a TW x TH BLOCK of pixels, not a run of a raster line: the simplex vertices of a pixel are shared with its
// neighbours in both directions (Gaussian cells are 3 px wide, lattice points are numbered along a Z-order curve), so a block
// touches about half the distinct value rows of a strip of the same size and the slice gathers hit L1 / L2 accordingly.
// WIDE (rows of >= CRF_WAVE_SOFTMAX_K channels per group): the wave-parallel softmax below; such tiles are LDS-bound to three
// workgroups per CU, so the kernel may use 128 registers (the narrow form is held to 80 for six waves per SIMD: 714 -> 607 us
// per launch on the headline batch, of which 714 -> 648 at five waves from the leaner record staging and store loop below).
// Tile geometry, item walk, record staging, slice, label and store loop are the pieces of crf_tile.h, shared with the kernels
// below; the two softmax forms, thread per row and wave per rows, are this kernel's own.
template <bool WIDE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WIDE ? 4 : 6)))
void crf_update_kernel(const CrfLattice Lg, const CrfLattice Lb, const PostDesc* __restrict__ imgs,
                                                         const float* __restrict__ vg, const float* __restrict__ vb,
                                                         const float* __restrict__ norm_g, const float* __restrict__ norm_b,
                                                         const float* __restrict__ unary, float* __restrict__ Q, float w_g,
                                                         float w_b, float alpha_g, float alpha_b, int pairwise, int img0,
                                                         int nimg, int tp_cap, int tile_w, const CrfLabelOut lout) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // [TP][Kp + 1], then the slice records [TP][20]
    // XCD-affine sweep like the splat / blur kernels: the slice gathers of an image hit the value rows
    // its XCD has just blurred
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int tid = threadIdx.x;
    int b, part, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part, parts); wi++) {
        const PostDesc im = imgs[b];
        const int K = im.K, Kp = im.Kp, K4 = Kp >> 2, ldt = Kp + 1;
        f32x4* Q4 = reinterpret_cast<f32x4*>(Q + im.qoff);
        // (the same in every lane; said so, because a load under a condition is a per-lane load to the compiler)
        const int lo_g = __builtin_amdgcn_readfirstlane(pairwise ? Lg.idbase[b] : 0);
        const int lo_b = __builtin_amdgcn_readfirstlane(pairwise ? Lb.idbase[b] : 0);
        const int TPe = CRF_TP / im.G < tp_cap ? CRF_TP / im.G : tp_cap; // one softmax thread per (pixel, group)
        const int TW = tile_w > 0 ? tile_w : crf_tile_w(TPe), TH = TPe / TW, TP = TW * TH;   // TW: a power of two
        const int tw_shift = __ffs(TW) - 1;
        const CrfTiles tiles = crf_tiles(im, TW, TH);
        const CrfShare sh = crf_share(tiles.ntiles, part, parts);
        // rows of the pixel-major arrays and of the lattice value arrays as base + 32-bit byte offset
        const char* const Ub = reinterpret_cast<const char*>(unary + im.qoff);
        const char* const Gb = reinterpret_cast<const char*>(vg + im.voff[0]);
        const char* const Bb = reinterpret_cast<const char*>(vb + im.voff[1]);
        const uint32_t rowb = (uint32_t)K4 * 16u;
        int* const rec_ob = reinterpret_cast<int*>(tile + TP * ldt);                   // [TP][6] bilateral ids, then ...
        float* const rec_wb = reinterpret_cast<float*>(rec_ob + TP * 6);
        int* const rec_og = reinterpret_cast<int*>(rec_wb + TP * 6);
        float* const rec_wg = reinterpret_cast<float*>(rec_og + TP * 3);
        float* const rec_nb = rec_wg + TP * 3;
        float* const rec_ng = rec_nb + TP;
        const CrfItemWalk it0(tid, K4);
        for (int tl = sh.first + slot; tl < sh.end; tl += bpx) {
            const CrfTileAt at = tiles.at(tl, TW, TH, tw_shift, im);
            // the tile's per-pixel slice records -- 6 + 3 image-local lattice ids and barycentric weights, two normalisers --
            // are staged once through LDS instead of being fetched by every channel-chunk lane of the pixel: 10 vector-memory
            // instructions per (pixel, chunk) item instead of 30 (the kernel is issue-bound there).  One thread per pixel: its
            // 6 + 6 + 3 + 3 words are consecutive (wide loads), and no per-thread division by 6 / 3 is carried through the tile
            // loop in registers
            if (pairwise) {
                for (int pl = tid; pl < TP; pl += 256) {                 // (TP <= 256: one pixel per thread)
                    const size_t g = (size_t)im.pix0 + at.pixel_of(pl);
                    crf_stage_record<6>(Lb, lo_b, g, pl, rec_ob, rec_wb);
                    crf_stage_record<3>(Lg, lo_g, g, pl, rec_og, rec_wg);
                    rec_nb[pl] = norm_b[g];
                    rec_ng[pl] = norm_g[g];
                }
                __syncthreads();
            }
            for (CrfItemWalk it = it0; it.item < TP * K4; it.next()) {
                const int pl = it.pl, c = it.c, px = at.pixel_of(pl);
                const uint32_t cofs = (uint32_t)c * 16u;
                const f32x4 u = ld_stream(reinterpret_cast<const f32x4*>(Ub + (__umul24((uint32_t)px, rowb) + cofs)));
                f32x4 t = {-u[0], -u[1], -u[2], -u[3]};
                if (pairwise) {
                    f32x4 vg3[3], vb6[6];
                    crf_gather_rows<3>(Gb, rec_og + pl * 3, rowb, cofs, vg3);
                    crf_gather_rows<6>(Bb, rec_ob + pl * 6, rowb, cofs, vb6);
                    const f32x4 og = crf_slice_rows<3>(vg3, rec_wg + pl * 3, alpha_g);
                    const float nrg = rec_ng[pl];
#pragma unroll
                    for (int i = 0; i < 4; i++) t[i] = __fsub_rn(t[i], __fmul_rn(-w_g, __fmul_rn(og[i], nrg)));
                    const f32x4 ob = crf_slice_rows<6>(vb6, rec_wb + pl * 6, alpha_b);
                    const float nrb = rec_nb[pl];
#pragma unroll
                    for (int i = 0; i < 4; i++) t[i] = __fsub_rn(t[i], __fmul_rn(-w_b, __fmul_rn(ob[i], nrb)));
                }
#pragma unroll
                for (int i = 0; i < 4; i++) tile[pl * ldt + 4 * c + i] = t[i];
            }
            __syncthreads();
            if (WIDE && K >= CRF_WAVE_SOFTMAX_K) {                       // (per image: the rows of a batch differ in width)
                // Wide rows (round 6): the softmax of a tile's rows by WAVE, not by thread.  With one thread per (pixel, group) a
                // 32-pixel tile of 2 x 150 channels keeps ONE wave busy for ~6000 dependent instructions per lane (150 exponentials
                // in a row) while the other three idle.  Here each wave owns RW = TP * G / 4 rows and works through them without any
                // workgroup barrier: maxima and exponentials with the lanes over the CHANNELS of one row at a time (the maximum is
                // order-independent, pnp_expf is a pure function), the sums -- the one order-dependent step, k = 0 .. K - 1 as
                // densecrf's expAndNormalize adds them -- with one LANE PER ROW, sequentially, all rows of the wave at once; then the
                // divisions with the lanes over the channels again.  Element by element the arithmetic of the thread-per-row form:
                // bit-identical marginals and labels.  (Narrower rows keep that form: measured slower there, see CRF_WAVE_SOFTMAX_K.)  Cross-lane hand-over through LDS inside one wave needs no barrier: a wave's LDS
                // operations execute in order.
                const int lane = tid & 63, wave = tid >> 6;
                const int R = TP * im.G, RW = R >> 2;                   // rows (pixel, group) of the tile / per wave: 4 .. 64
                const int rbase = wave * RW;
                auto row_ptr = [&](int rr) {                            // row rr of the tile: group-major like the thread form
                    const int grp = rr / TP, px = rr - grp * TP;
                    return tile + px * ldt + grp * im.Kg;
                };
                float s_mine = 0.f;                                     // lane j < RW: sum of row rbase + j
                // pass 1: per row, maximum (NaN if any NaN) and exponentials, lanes over channels; two rows at a time (RW is even), so
                // that one row's shuffle chain runs under the other's loads and exponentials
                for (int j = 0; j < RW; j += 2) {
                    float* const row0 = row_ptr(rbase + j);
                    float* const row1 = row_ptr(rbase + j + 1);
                    float m0 = -INFINITY, m1 = -INFINITY;
                    bool nan0 = false, nan1 = false;
                    for (int k = lane; k < K; k += 64) {
                        const float v0 = row0[k], v1 = row1[k];
                        nan0 |= v0 != v0;
                        nan1 |= v1 != v1;
                        m0 = v0 > m0 ? v0 : m0;
                        m1 = v1 > m1 ? v1 : m1;
                    }
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) {
                        const float a0 = __shfl_xor(m0, o, 64), a1 = __shfl_xor(m1, o, 64);
                        m0 = a0 > m0 ? a0 : m0;
                        m1 = a1 > m1 ? a1 : m1;
                    }
                    if (__any(nan0)) m0 = __builtin_nanf("");
                    if (__any(nan1)) m1 = __builtin_nanf("");
                    for (int k = lane; k < K; k += 64) {
                        const float e0 = pnp_expf(__fsub_rn(row0[k], m0)), e1 = pnp_expf(__fsub_rn(row1[k], m1));
                        row0[k] = e0;
                        row1[k] = e1;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                // pass 2: sums in channel order, one lane per row
                if (lane < RW) {
                    const float* row = row_ptr(rbase + lane);
                    float sm = 0.f;
                    for (int k = 0; k < K; k++) sm = __fadd_rn(sm, row[k]);
                    s_mine = sm;
                }
                // pass 3: divisions, lanes over channels
                for (int j = 0; j < RW; j++) {
                    float* row = row_ptr(rbase + j);
                    const float sm = __shfl(s_mine, j, 64);
                    for (int k = lane; k < K; k += 64) row[k] = __fdiv_rn(row[k], sm);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (lane < RW) {
                    const int rr = rbase + lane, grp = rr / TP, px = rr - grp * TP;
                    float* row = tile + px * ldt + grp * im.Kg;
                    crf_store_label(lout, grp, b, at, px, row, K);         // (last iteration)
                    if (grp == im.G - 1)                                // pad floats behind the last group stay zero
                        for (int k = im.G * im.Kg; k < Kp; k++) tile[px * ldt + k] = 0.f;
                }
            } else if (tid < TP * im.G) {                               // one softmax per (pixel, channel group)
                const int grp = tid / TP, px = tid - grp * TP;
                {
                    float* row = tile + px * ldt + grp * im.Kg;
                    float m = row[0];
                    for (int k = 1; k < K; k++) {
                        const float v = row[k];
                        if (v > m || v != v) m = v;
                    }
                    float s = 0.f;
                    for (int k = 0; k < K; k++) {
                        const float e = pnp_expf(__fsub_rn(row[k], m));
                        row[k] = e;
                        s = __fadd_rn(s, e);
                    }
                    for (int k = 0; k < K; k++) row[k] = __fdiv_rn(row[k], s);
                    crf_store_label(lout, grp, b, at, px, row, K);         // (last iteration)
                    if (grp == im.G - 1)                                // pad floats behind the last group stay zero
                        for (int k = im.G * im.Kg; k < Kp; k++) tile[px * ldt + k] = 0.f;
                }
            }
            __syncthreads();
            crf_store_tile<true>(tile, ldt, at, it0, TP, Q4);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------
// The update with label-compatibility MATRICES (the stand-alone solver, crf_op.hip; the engine's Potts runs never come here):
//   acc_t[l] = sum_k M_t[l][k] * msg_t[k]   (one fp32 accumulator per output, k ascending, multiply and add rounded
//                                            separately: no FMA, no MFMA -- the order of the sum is part of the contract)
//   logit[l] = (-U[l] + acc_g[l]) + acc_b[l],   Q = softmax(logit)
// msg_t[k] is what crf_update_kernel forms per term -- (sum_v (bary_v * val_v[k]) * alpha_t) * norm_t, the statements of
// crf_gather_rows / crf_slice_rows in their order -- so M_t = w * I gives the Potts kernel's logits value for value (the other
// products are exact zeros).  Same TW x TH block tiles, LDS-staged slice records, XCD-affine sweep and 16-byte global I/O as
// crf_update_kernel, but WRITTEN OUT here, not called from crf_tile.h: with the pieces the compiler scheduled the scalar loads
// of phase 2's inner loop differently and the K = 150 update ran 3.7 - 4.5 % slower (profiles/crf_update_pieces.txt; no single
// piece does it).  A change to a piece is repeated here by hand; tests/test_crf_general_gpu.py and test_crf_terms_gpu.py hold
// this kernel to the others bit for bit.  Phase 1 (lanes over (pixel, 16-byte chunk) items) puts -U into the logit tile and
// the two message rows of every pixel into LDS (row stride Kp + 1: odd, so the per-pixel reads of phase 2 hit 32 distinct
// banks per half wave).  Phase 2 does
// the two K x K products with lane = pixel: a wave owns 64 pixels (32 where a tile has only 32: half the lanes idle) and a
// block of CRF_CL labels l at a time, so every M_t[l][k] is the same in all lanes and is read with scalar loads from global
// memory (two 150 x 150 matrices are 180 KB: not LDS material), and one LDS read of msg_t[k] feeds CRF_CL accumulators.  The
// matrices arrive TRANSPOSED (MgT[k * ldm + l] = M_g[l][k]; ldm a multiple of CRF_CL, zero beyond K), so the CRF_CL weights a
// block needs for one k are 32 consecutive bytes -- one scalar load and one pointer per term -- and a block that reaches past K
// multiplies by the pad's zeros into accumulators nobody reads.  The
// blocks of l are dealt round the 4 / (TP / 64) waves that share a pixel set.  Then softmax, labels and the zeroing of the pad
// floats with crf_update_kernel's thread-per-row arithmetic, and its store loop.
// Tile size (crf_update_compat): 256 / 128 pixels while the three LDS rows per pixel stay under 64 KB (Kp <= 12 / <= 32), 64
// up to Kp = 200, 32 beyond (three rows of 257 floats x 64 pixels would pass the CU's 160 KB).
// KL = true: no update.  The tile holds Q instead of -U and a fourth row per pixel holds U; phase 2 ends in the pixel's term of
// pnp_crf_kl, sum_l q log(max(q, 1e-20)) + q U[l] - q acc_g[l] - q acc_b[l] (products fp32, summed in fp64 in this order: l
// ascending inside a wave's label blocks, then the waves of the pixel in order), written to kl_pix[pixel].
// Compiler's resource report for gfx950 (-Rpass-analysis=kernel-resource-usage): update form 92 VGPRs, 106 SGPRs, no scratch
// (101 scalar registers spilled to vector-register lanes); KL form 99 / 106, no scratch.  Five (KL: four)
// waves per SIMD by registers, but the tile's LDS decides: 35 KB at K = 3
// (256 pixels) and 33 KB at K = 33 (64 pixels) leave four workgroups = four waves per SIMD, 48 KB at K = 21 (128 pixels) three,
// 120 KB at K = 150 (64 pixels) one.  The inner loop is packed fp32 multiplies and adds (v_pk_mul_f32 / v_pk_add_f32, each
// rounded on its own) fed by s_load_dwordx8 and ds_read2_b32.  No rate is claimed: tools/crf_bench.py --compat matrix measures.
template <bool KL>
__global__ __launch_bounds__(256) void crf_update_compat_kernel(const CrfLattice Lg, const CrfLattice Lb, const PostDesc* __restrict__ imgs,
                                                                const float* __restrict__ vg, const float* __restrict__ vb,
                                                                const float* __restrict__ norm_g, const float* __restrict__ norm_b,
                                                                const float* __restrict__ unary, float* Q, const float* __restrict__ MgT,
                                                                const float* __restrict__ MbT, int ldm, float alpha_g, float alpha_b,
                                                                int img0, int nimg, int TP, const CrfLabelOut lout,
                                                                double* __restrict__ kl_pix) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // [TP][Kp + 1] x 3 (KL: x 4), then the slice records [TP][20]
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int TW = crf_tile_w(TP), TH = TP / TW;                        // TP = 32 .. 256, a power of two
    const int tw_shift = __ffs(TW) - 1;
    // phase 2: WPS waves cover the pixels of a tile, NG = 4 / WPS waves share a pixel set and split the labels
    const int WPS = TP > 64 ? TP >> 6 : 1, NG = 4 / WPS;
    const int px2 = (wave % WPS) * 64 + lane, lg = wave / WPS;
    const bool act = px2 < TP;
    const int pxc = act ? px2 : TP - 1;                                 // idle lanes read a valid row and write nothing
    int b, part, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part, parts); wi++) {
        const PostDesc im = imgs[b];
        const int K = im.K, Kp = im.Kp, K4 = Kp >> 2, ldt = Kp + 1;
        f32x4* Q4 = reinterpret_cast<f32x4*>(Q + im.qoff);
        const int lo_g = Lg.idbase[b], lo_b = Lb.idbase[b];
        const int tiles_x = (im.W + TW - 1) / TW, tiles_y = (im.H + TH - 1) / TH, ntiles = tiles_x * tiles_y;
        const int tfirst = (int)((long)ntiles * part / parts), tend = (int)((long)ntiles * (part + 1) / parts);
        const char* const Ub = reinterpret_cast<const char*>(unary + im.qoff);
        const char* const Gb = reinterpret_cast<const char*>(vg + im.voff[0]);
        const char* const Bb = reinterpret_cast<const char*>(vb + im.voff[1]);
        const uint32_t rowb = (uint32_t)K4 * 16u;
        float* const msg_g = tile + TP * ldt;
        float* const msg_b = msg_g + TP * ldt;
        float* const ubuf = msg_b + TP * ldt;                                          // (KL only)
        int* const rec_ob = reinterpret_cast<int*>(msg_b + (KL ? 2 : 1) * TP * ldt);   // [TP][6] bilateral ids, then ...
        float* const rec_wb = reinterpret_cast<float*>(rec_ob + TP * 6);
        int* const rec_og = reinterpret_cast<int*>(rec_wb + TP * 6);
        float* const rec_wg = reinterpret_cast<float*>(rec_og + TP * 3);
        float* const rec_nb = rec_wg + TP * 3;
        float* const rec_ng = rec_nb + TP;
        const int q256 = 256 / K4, r256 = 256 - q256 * K4;
        const int pl0 = tid / K4, c0 = tid - pl0 * K4;
        for (int tl = tfirst + slot; tl < tend; tl += bpx) {
            const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
            const int x0 = tx * TW, y0 = ty * TH;
            auto pixel_of = [&](int pl) {
                const int x = x0 + (pl & (TW - 1)), y = y0 + (pl >> tw_shift);
                return (y < im.H ? y : im.H - 1) * im.W + (x < im.W ? x : im.W - 1);
            };
            auto inside = [&](int pl) { return x0 + (pl & (TW - 1)) < im.W && y0 + (pl >> tw_shift) < im.H; };
            for (int pl = tid; pl < TP; pl += 256) {                     // slice records, one pixel per thread
                const size_t g = (size_t)im.pix0 + pixel_of(pl);
#pragma unroll
                for (int v = 0; v < 6; v++) {
                    rec_ob[pl * 6 + v] = Lb.offset[g * 6 + v] - lo_b;
                    rec_wb[pl * 6 + v] = Lb.bary[g * 6 + v];
                }
#pragma unroll
                for (int v = 0; v < 3; v++) {
                    rec_og[pl * 3 + v] = Lg.offset[g * 3 + v] - lo_g;
                    rec_wg[pl * 3 + v] = Lg.bary[g * 3 + v];
                }
                rec_nb[pl] = norm_b[g];
                rec_ng[pl] = norm_g[g];
            }
            __syncthreads();
            {   // phase 1: -U (KL: Q, U) and the two message rows of every pixel -> LDS
                int pl = pl0, c = c0;
                for (int item = tid; item < TP * K4; item += 256) {
                    const int px = pixel_of(pl);
                    const uint32_t cofs = (uint32_t)c * 16u;
                    const f32x4 u = ld_stream(reinterpret_cast<const f32x4*>(Ub + (__umul24((uint32_t)px, rowb) + cofs)));
                    f32x4 t = {-u[0], -u[1], -u[2], -u[3]};
                    if (KL) t = Q4[(size_t)px * K4 + c];
                    f32x4 vg3[3], vb6[6];
#pragma unroll
                    for (int v = 0; v < 3; v++)
                        vg3[v] = *reinterpret_cast<const f32x4*>(Gb + (__umul24((uint32_t)rec_og[pl * 3 + v], rowb) + cofs));
#pragma unroll
                    for (int v = 0; v < 6; v++)
                        vb6[v] = *reinterpret_cast<const f32x4*>(Bb + (__umul24((uint32_t)rec_ob[pl * 6 + v], rowb) + cofs));
                    f32x4 og = {0.f, 0.f, 0.f, 0.f}, ob = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int v = 0; v < 3; v++) {
                        const float wv = rec_wg[pl * 3 + v];
#pragma unroll
                        for (int i = 0; i < 4; i++) og[i] = __fadd_rn(og[i], __fmul_rn(__fmul_rn(wv, vg3[v][i]), alpha_g));
                    }
#pragma unroll
                    for (int v = 0; v < 6; v++) {
                        const float wv = rec_wb[pl * 6 + v];
#pragma unroll
                        for (int i = 0; i < 4; i++) ob[i] = __fadd_rn(ob[i], __fmul_rn(__fmul_rn(wv, vb6[v][i]), alpha_b));
                    }
                    const float nrg = rec_ng[pl], nrb = rec_nb[pl];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        tile[pl * ldt + 4 * c + i] = t[i];
                        msg_g[pl * ldt + 4 * c + i] = __fmul_rn(og[i], nrg);
                        msg_b[pl * ldt + 4 * c + i] = __fmul_rn(ob[i], nrb);
                        if (KL) ubuf[pl * ldt + 4 * c + i] = u[i];
                    }
                    pl += q256;
                    c += r256;
                    if (c >= K4) {
                        c -= K4;
                        pl++;
                    }
                }
            }
            __syncthreads();
            // phase 2: lane = pixel, CRF_CL labels per pass over k; M rows through scalar loads (l0, K, ldm are wave-uniform)
            double kl = 0.0;
            {
                const float* const xg = msg_g + pxc * ldt;
                const float* const xb = msg_b + pxc * ldt;
                for (int l0 = lg * CRF_CL; l0 < K; l0 += NG * CRF_CL) {
                    float ag[CRF_CL], ab[CRF_CL];
#pragma unroll
                    for (int i = 0; i < CRF_CL; i++) ag[i] = ab[i] = 0.f;
                    // the block's weights of one k: 32 consecutive bytes of the transposed matrix (labels past K: its zero pad)
                    const float* tg = MgT + l0;
                    const float* tb = MbT + l0;
#pragma unroll 4
                    for (int k = 0; k < K; k++) {
                        const float mg = xg[k], mb = xb[k];
#pragma unroll
                        for (int i = 0; i < CRF_CL; i++) {
                            ag[i] = __fadd_rn(ag[i], __fmul_rn(tg[i], mg));
                            ab[i] = __fadd_rn(ab[i], __fmul_rn(tb[i], mb));
                        }
                        tg += ldm;
                        tb += ldm;
                    }
#pragma unroll
                    for (int i = 0; i < CRF_CL; i++) {
                        if (act && l0 + i < K) {
                            float* const t = tile + px2 * ldt + l0 + i;
                            if (KL) {
                                const float q = *t, qc = q > 1e-20f ? q : 1e-20f;
                                kl += (double)__fmul_rn(q, pnp_logf(qc));
                                kl += (double)__fmul_rn(q, ubuf[px2 * ldt + l0 + i]);
                                kl -= (double)__fmul_rn(q, ag[i]);
                                kl -= (double)__fmul_rn(q, ab[i]);
                            } else {
                                *t = __fadd_rn(__fadd_rn(*t, ag[i]), ab[i]);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            if (KL) {
                double* const part_kl = reinterpret_cast<double*>(msg_g);      // [NG][TP]: the message rows are spent
                if (act) part_kl[lg * TP + px2] = kl;
                __syncthreads();
                if (tid < TP && inside(tid)) {
                    double e = 0.0;
                    for (int g = 0; g < NG; g++) e += part_kl[g * TP + tid];
                    kl_pix[(size_t)im.pix0 + pixel_of(tid)] = e;
                }
                __syncthreads();
                continue;
            }
            // softmax, label, pad: element by element the arithmetic of crf_update_kernel's thread-per-row form.  The two steps
            // that depend on the order along a row -- the maximum as that form finds it (a NaN wins) and the sum, k ascending --
            // stay with one thread per row; the exponentials and the divisions, pure functions of one element, go to the lanes of
            // phase 2 (pixel, wave of the pixel set), so a 64-pixel tile keeps four waves busy with them, not one.  Row maximum
            // and sum pass through the spent normaliser slots of the slice records
            if (tid < TP) {
                const float* row = tile + tid * ldt;
                float m = row[0];
                for (int k = 1; k < K; k++) {
                    const float v = row[k];
                    if (v > m || v != v) m = v;
                }
                rec_ng[tid] = m;
            }
            __syncthreads();
            if (act) {
                float* row = tile + px2 * ldt;
                const float m = rec_ng[px2];
                for (int k = lg; k < K; k += NG) row[k] = pnp_expf(__fsub_rn(row[k], m));
            }
            __syncthreads();
            if (tid < TP) {
                const float* row = tile + tid * ldt;
                float s = 0.f;
                for (int k = 0; k < K; k++) s = __fadd_rn(s, row[k]);
                rec_ng[tid] = s;
            }
            __syncthreads();
            if (act) {
                float* row = tile + px2 * ldt;
                const float s = rec_ng[px2];
                for (int k = lg; k < K; k += NG) row[k] = __fdiv_rn(row[k], s);
            }
            __syncthreads();
            if (tid < TP) {
                const int px = tid;
                float* row = tile + px * ldt;
                if (lout.lab[0]) {                                       // first maximum, NaN counts as maximum (np.argmax)
                    int best = 0;
                    float bv = row[0];
                    for (int k = 1; k < K; k++) {
                        const float v = row[k];
                        if (bv == bv && (v > bv || v != v)) {
                            best = k;
                            bv = v;
                        }
                    }
                    if (inside(px)) lout.lab[0][lout.label_off[b] + pixel_of(px)] = (uint8_t)lout.lut[b * lout.lut_stride + best];
                }
                for (int k = K; k < Kp; k++) row[k] = 0.f;               // pad floats stay zero
            }
            __syncthreads();
            {
                int pl = pl0, c = c0;
                for (int item = tid; item < TP * K4; item += 256) {
                    if (inside(pl)) {
                        const float* r = tile + pl * ldt + 4 * c;
                        st_stream(Q4 + (size_t)pixel_of(pl) * K4 + c, f32x4{r[0], r[1], r[2], r[3]});
                    }
                    pl += q256;
                    c += r256;
                    if (c >= K4) {
                        c -= K4;
                        pl++;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------
// One pairwise term of a T-term update over caller-supplied features (pnp_crf_set_batch_terms; the two-term runs above never come
// here): slice the term's blurred lattice (D1 = d + 1 = 2 .. 7 vertices per pixel), weigh the message, add it into the
// pixel-major logit row, and after the last term take the softmax:
//   msg[k]   = (sum_v (bary_v * val_v[k]) * alpha) * norm        crf_gather_rows / crf_slice_rows<D1>
//   acc[l]   = w * msg[l] | wvec[l] * msg[l] | sum_k M[l][k] * msg[k]      (one fp32 accumulator, k ascending, no FMA)
//   row[l]   = (first ? -U[l] : row[l]) + acc[l]
//   last:  Q = softmax(row), labels, zero pad -- crf_update_compat_kernel's arithmetic element by element
// so T = 2 with xy and xy+rgb features leaves the bits of crf_update_kernel (scalars: the same functions for 3 and 6 vertices)
// / crf_update_compat_kernel (matrices: the same statements, written out there).  The other pieces of crf_tile.h: TW x TH
// pixel tiles, slice records (2 D1 + 1 words per pixel) staged in LDS by one thread per pixel, 16-byte row gathers with lanes
// over (pixel, chunk) items, wave roles of phase 2, store loop; XCD-affine image schedule.  `base` and `out` may be the
// same array (the logit rows, updated in place: an item reads its chunk before it writes it, and a tile's rows are only its
// own).  What a launch keeps in LDS besides the records: nothing (scalar / vector weights, not last: rows go from registers
// straight to memory), the logit tile (last: the softmax needs whole rows), or tile + message rows (MATRIX: phase 2 with
// lane = pixel and the transposed matrix through scalar loads: crf_update_compat_kernel's, written out for one term).
// imgs: the TERM's descriptors (voff[0] = its value rows).
// Per-thread arrays are indexed by unrolled loops over the template's D1 only.
template <int D1, bool MATRIX>
__global__ __launch_bounds__(256) void crf_term_update_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs, const float* __restrict__ val,
                                                              const float* __restrict__ norm, const float* base, int first, float* out, int last,
                                                              float w, const float* __restrict__ wvec, const float* __restrict__ MT, int ldm,
                                                              float alpha, int img0, int nimg, int TP, const CrfLabelOut lout) {
    extern __shared__ __attribute__((aligned(16))) float tile[];        // [TP][Kp + 1] x (0 | 1 | 2), then the slice records
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const int tid = threadIdx.x;
    const bool tiled = MATRIX || last;
    const int TW = crf_tile_w(TP), TH = TP / TW;                        // TP = 32 .. 256, a power of two
    const int tw_shift = __ffs(TW) - 1;
    const CrfWaveRole wr = crf_wave_role(TP, tid);                      // phase 2 and the softmax
    int b, part, parts;
    for (int wi = 0; xcd_work(wi, xcd, img0, nimg, b, part, parts); wi++) {
        const PostDesc im = imgs[b];
        const int K = im.K, Kp = im.Kp, K4 = Kp >> 2, ldt = Kp + 1;
        const int lo = L.idbase[b];
        const CrfTiles tiles = crf_tiles(im, TW, TH);
        const CrfShare sh = crf_share(tiles.ntiles, part, parts);
        const char* const Bb = reinterpret_cast<const char*>(base + im.qoff);
        const char* const Vb = reinterpret_cast<const char*>(val + im.voff[0]);
        f32x4* const O4 = reinterpret_cast<f32x4*>(out + im.qoff);
        const uint32_t rowb = (uint32_t)K4 * 16u;
        float* const msg = tile + TP * ldt;                                            // (MATRIX only)
        int* const rec_o = reinterpret_cast<int*>(tile + ((tiled ? 1 : 0) + (MATRIX ? 1 : 0)) * TP * ldt);   // [TP][D1] lattice ids
        float* const rec_w = reinterpret_cast<float*>(rec_o + TP * D1);                // [TP][D1] barycentric weights
        float* const rec_n = rec_w + TP * D1;                                          // [TP] normaliser; then row maximum / sum
        const CrfItemWalk it0(tid, K4);
        for (int tl = sh.first + slot; tl < sh.end; tl += bpx) {
            const CrfTileAt at = tiles.at(tl, TW, TH, tw_shift, im);
            for (int pl = tid; pl < TP; pl += 256) {                     // slice records, one pixel per thread
                const size_t g = (size_t)im.pix0 + at.pixel_of(pl);
                crf_stage_record<D1>(L, lo, g, pl, rec_o, rec_w);
                rec_n[pl] = norm[g];
            }
            __syncthreads();
            // phase 1: the message chunk of every (pixel, chunk) item; without a matrix also its weight and the row's sum
            for (CrfItemWalk it = it0; it.item < TP * K4; it.next()) {
                const int pl = it.pl, c = it.c, px = at.pixel_of(pl);
                const uint32_t cofs = (uint32_t)c * 16u;
                f32x4 t = *reinterpret_cast<const f32x4*>(Bb + (__umul24((uint32_t)px, rowb) + cofs));
                if (first) t = f32x4{-t[0], -t[1], -t[2], -t[3]};
                f32x4 vv[D1];
                crf_gather_rows<D1>(Vb, rec_o + pl * D1, rowb, cofs, vv);
                const f32x4 o = crf_slice_rows<D1>(vv, rec_w + pl * D1, alpha);
                const float nr = rec_n[pl];
                f32x4 m;
#pragma unroll
                for (int i = 0; i < 4; i++) m[i] = __fmul_rn(o[i], nr);
                if (!MATRIX) {
                    f32x4 wl = {w, w, w, w};
                    if (wvec) wl = *reinterpret_cast<const f32x4*>(wvec + 4 * c);
#pragma unroll
                    for (int i = 0; i < 4; i++) t[i] = __fadd_rn(t[i], __fmul_rn(wl[i], m[i]));
                }
                if (tiled) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        tile[pl * ldt + 4 * c + i] = t[i];
                        if (MATRIX) msg[pl * ldt + 4 * c + i] = m[i];
                    }
                } else if (at.inside(pl)) {
                    O4[(size_t)px * K4 + c] = t;
                }
            }
            __syncthreads();
            if (!tiled) continue;
            if (MATRIX) {   // phase 2: lane = pixel, CRF_CL labels per pass over k; M rows through scalar loads (wave-uniform)
                const float* const x = msg + wr.pxc * ldt;
                for (int l0 = wr.lg * CRF_CL; l0 < K; l0 += wr.NG * CRF_CL) {
                    float a[CRF_CL];
#pragma unroll
                    for (int i = 0; i < CRF_CL; i++) a[i] = 0.f;
                    const float* tm = MT + l0;                           // (labels past K: the zero pad of the transposed matrix)
#pragma unroll 4
                    for (int k = 0; k < K; k++) {
                        const float mk = x[k];
#pragma unroll
                        for (int i = 0; i < CRF_CL; i++) a[i] = __fadd_rn(a[i], __fmul_rn(tm[i], mk));
                        tm += ldm;
                    }
#pragma unroll
                    for (int i = 0; i < CRF_CL; i++) {
                        if (wr.act && l0 + i < K) {
                            float* const t = tile + wr.px2 * ldt + l0 + i;
                            *t = __fadd_rn(*t, a[i]);
                        }
                    }
                }
                __syncthreads();
            }
            if (last) {
                // softmax, label, pad: crf_update_compat_kernel's steps, element by element -- maximum (a NaN wins) and sum
                // (k ascending) by one thread per row, exponentials and divisions by the lanes of phase 2; row maximum and sum
                // pass through the spent normaliser slots
                if (tid < TP) {
                    const float* row = tile + tid * ldt;
                    float mx = row[0];
                    for (int k = 1; k < K; k++) {
                        const float v = row[k];
                        if (v > mx || v != v) mx = v;
                    }
                    rec_n[tid] = mx;
                }
                __syncthreads();
                if (wr.act) {
                    float* row = tile + wr.px2 * ldt;
                    const float mx = rec_n[wr.px2];
                    for (int k = wr.lg; k < K; k += wr.NG) row[k] = pnp_expf(__fsub_rn(row[k], mx));
                }
                __syncthreads();
                if (tid < TP) {
                    const float* row = tile + tid * ldt;
                    float sm = 0.f;
                    for (int k = 0; k < K; k++) sm = __fadd_rn(sm, row[k]);
                    rec_n[tid] = sm;
                }
                __syncthreads();
                if (wr.act) {
                    float* row = tile + wr.px2 * ldt;
                    const float sm = rec_n[wr.px2];
                    for (int k = wr.lg; k < K; k += wr.NG) row[k] = __fdiv_rn(row[k], sm);
                }
                __syncthreads();
                if (tid < TP) {
                    float* row = tile + tid * ldt;
                    crf_store_label(lout, 0, b, at, tid, row, K);
                    for (int k = K; k < Kp; k++) row[k] = 0.f;           // pad floats stay zero
                }
                __syncthreads();
            }
            if (last) crf_store_tile<true>(tile, ldt, at, it0, TP, O4);
            else crf_store_tile<false>(tile, ldt, at, it0, TP, O4);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------ host
// the splat of crf_filter: va = S N rows, for rows of up to max_kp floats
static void crf_splat(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* Q, float* va, int max_kp, hipStream_t s) {
    const int k4 = (max_kp + 3) / 4;
#define PNP_SPLAT(LPP_, MULTI_)                                                                                                  \
    do {                                                                                                                      \
        static PerDeviceInt g0_, g1_;                        /* per device ordinal (common.h) */                              \
        const int nbs0 = g0_.get([] { return resident_grid(crf_splat_kernel<LPP_, 0, MULTI_>, 256, 0); });                    \
        const int nbs1 = g1_.get([] { return resident_grid(crf_splat_kernel<LPP_, 1, MULTI_>, 256, 0); });                    \
        if (L.which == 0) hipLaunchKernelGGL((crf_splat_kernel<LPP_, 0, MULTI_>), dim3(nbs0), dim3(256), 0, s, L, d_imgs, Q, va, img0, nimg); \
        else hipLaunchKernelGGL((crf_splat_kernel<LPP_, 1, MULTI_>), dim3(nbs1), dim3(256), 0, s, L, d_imgs, Q, va, img0, nimg);              \
    } while (0)
    if (k4 <= 8) PNP_SPLAT(8, false);
    else if (k4 <= 16) PNP_SPLAT(16, false);
    else if (k4 <= 32) PNP_SPLAT(32, false);
    else PNP_SPLAT(32, true);
#undef PNP_SPLAT
}

// lattice(norm * Q) for images [img0, img0+nimg): splat + (d+1) blurs (the normaliser rides in the contributor records).
// reverse: lattice^T(norm * Q), the blur axes d, d - 1, .. 0 one crf_blur4_kernel pass each (the adjoint of the forward
// product of symmetric axis blurs).  Returns the buffer holding the result.  splat_only: the splatted rows, no axis.
int crf_filter(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* Q,
               float* va, float* vb, const float** result, int max_kp, hipStream_t s, bool reverse, bool splat_only) {
    const int D = L.D1 - 1;
    crf_splat(L, d_imgs, img0, nimg, Q, va, max_kp, s);
    if (splat_only) {
        *result = va;
        return ok();
    }
    static PerDeviceInt gb2, gb1;                            // per device ordinal (common.h)
    const int nb2 = gb2.get([] { return resident_grid(crf_blur4x2_kernel, 256, 0); });
    const int nb1 = gb1.get([] { return resident_grid(crf_blur4_kernel, 256, 0); });
    float* src = va;
    float* dst = vb;
    // forward: axes in pairs through the fused two-axis kernel (bilateral: 3 passes for 6 axes; Gaussian: one pair + one single):
    // mean-field 41.6 -> 37.0 ms per bench step, results bit-identical
    for (int j = reverse ? D : 0; reverse ? j >= 0 : j <= D;) {
        if (!reverse && j + 1 <= D) {
            hipLaunchKernelGGL(crf_blur4x2_kernel, dim3(nb2), dim3(256), 0, s, L, d_imgs, src, dst, j / 2, img0, nimg);
            j += 2;
        } else {
            hipLaunchKernelGGL(crf_blur4_kernel, dim3(nb1), dim3(256), 0, s, L, d_imgs, src, dst, j, img0, nimg);
            j += reverse ? -1 : 1;
        }
        float* t = src;
        src = dst;
        dst = t;
    }
    *result = src;
    return ok();
}

// Q <- softmax(-U - pairwise terms) (pairwise != 0) or softmax(-U) (pairwise == 0)
int crf_update(const CrfLattice& Lg, const CrfLattice& Lb, const PostDesc* d_imgs, int img0, int nimg, const float* vg,
               const float* vb, const float* norm_g, const float* norm_b, const float* unary, float* Q, float w_g,
               float w_b, int pairwise, int max_kp, int groups, hipStream_t s, const CrfLabelOut& labels) {
    // tile + per-pixel slice records; wide rows (150 classes) take fewer pixels per tile to stay inside the CU's 160 KB
    size_t tp = (size_t)(CRF_TP / (groups > 0 ? groups : 1));
    const size_t per_pixel = ((size_t)max_kp + 1 + 20) * sizeof(float);
    if (groups == 2 && tp > 64) tp = 64;                     // smaller tiles, more resident workgroups: 643 -> 624 us on the paired bench rows
    // wide rows: keep a tile under ~48 KB so that three workgroups stay resident per CU (the kernel waits on its row gathers;
    // measured per bench step: COCO-Object K = 81 70 -> 58 ms at 64 pixels, ADE20K K = 2 x 150 348 -> 278 ms at 32 pixels;
    // below 32 pixels the per-tile overheads win: 295 ms at 16, 389 ms at 8)
    while (tp > 16 && tp * per_pixel > 48 * 1024) tp >>= 1;
    if (tp * per_pixel > 158 * 1024) tp = 158 * 1024 / per_pixel;
    const int tile_w = 0;                                    // 0: crf_tile_w(pixels per tile)
    if (tp < 4) return PNP_ERR_ARG;
    const bool wide = max_kp / (groups > 0 ? groups : 1) >= CRF_WAVE_SOFTMAX_K;      // some image of the batch may have such rows
    return crf_launch_tiled(wide ? crf_update_kernel<true> : crf_update_kernel<false>, tp * per_pixel, s, Lg, Lb, d_imgs, vg, vb, norm_g,
                            norm_b, unary, Q, w_g, w_b, crf_alpha(2), crf_alpha(5), pairwise, img0, nimg, (int)tp, tile_w, labels);
}

// Pixels per tile of crf_update_compat_kernel for rows of up to max_kp floats (see there): a multiple of the 64 pixels a wave
// takes in phase 2 wherever the CU's LDS holds that many
int crf_compat_tile_pixels(int max_kp, bool kl) {
    const size_t per_pixel = ((size_t)(kl ? 4 : 3) * (max_kp + 1) + 20) * sizeof(float);
    int tp = 256;
    while (tp > 64 && tp * per_pixel > 64 * 1024) tp >>= 1;
    if (tp * per_pixel > 158 * 1024) tp = 32;
    return tp;
}

// Q <- softmax(-U + M_g msg_g + M_b msg_b) (kl_pix null), or the per-pixel terms of the KL divergence at the current Q into
// kl_pix (Q is only read).  MgT / MbT: the matrices transposed, MgT[k * ldm + l] = M_g[l][k], ldm >= max_kp a multiple of
// CRF_CL, zeros wherever l or k is not a label
int crf_update_compat(const CrfLattice& Lg, const CrfLattice& Lb, const PostDesc* d_imgs, int img0, int nimg, const float* vg,
                      const float* vb, const float* norm_g, const float* norm_b, const float* unary, float* Q, const float* MgT,
                      const float* MbT, int ldm, int max_kp, hipStream_t s, const CrfLabelOut& labels, double* kl_pix) {
    const bool kl = kl_pix != nullptr;
    const int tp = crf_compat_tile_pixels(max_kp, kl);
    const size_t smem = (size_t)tp * ((size_t)(kl ? 4 : 3) * (max_kp + 1) + 20) * sizeof(float);
    if (max_kp < 4 || max_kp > 256 || ldm < max_kp || ldm % CRF_CL != 0) return PNP_ERR_ARG;
    return crf_launch_tiled(kl ? crf_update_compat_kernel<true> : crf_update_compat_kernel<false>, smem, s, Lg, Lb, d_imgs, vg, vb, norm_g,
                            norm_b, unary, Q, MgT, MbT, ldm, crf_alpha(2), crf_alpha(5), img0, nimg, tp, labels, kl_pix);
}

// One term of a T-term update (crf_term_update_kernel).  d_imgs: the term's descriptors; val: its filtered values (crf_filter);
// base: the unary rows (first) or the logit rows; out: the logit rows, or Q (last).  MT non-null: the K x K message weights
// transposed as crf_update_compat takes them; else wvec non-null: one weight per label (ldm floats, zero beyond K); else w
int crf_term_update(const CrfLattice& L, const PostDesc* d_imgs, int img0, int nimg, const float* val, const float* norm, const float* base,
                    bool first, float* out, bool last, float w, const float* wvec, const float* MT, int ldm, int max_kp, hipStream_t s,
                    const CrfLabelOut& labels) {
    if (max_kp < 4 || max_kp > 256 || ((MT || wvec) && (ldm < max_kp || ldm % CRF_CL != 0))) return PNP_ERR_ARG;
    return crf_dispatch<2, 7>(L.D1, [&](auto d1) {
        constexpr int D1 = decltype(d1)::value;
        size_t smem = 0;                                      // LDS rows per pixel: the message rows (matrix), the logit tile (matrix, last)
        const int tp = crf_term_tile_pixels(max_kp, D1, (MT ? 1 : 0) + (MT || last ? 1 : 0), &smem);
        return crf_launch_tiled(MT ? crf_term_update_kernel<D1, true> : crf_term_update_kernel<D1, false>, smem, s, L, d_imgs, val, norm, base,
                                first ? 1 : 0, out, last ? 1 : 0, w, wvec, MT, ldm, crf_alpha(D1 - 1), img0, nimg, tp, labels);
    });
}

}  // namespace pnp
