// Internal to csrc/, included only by crf_meanfield.hip and crf_grad.hip: the device pieces that the tiled kernels of those units
// -- crf_update_kernel, crf_term_update_kernel, crf_term_backward_kernel, crf_slice_add_kernel -- are put together from.  The
// tests hold those kernels to each other bit for bit (T = 2 scalar feature terms equal the Potts kernel); they agree because
// they call the same function, so a change to the slice sequence or the edge-tile rule is made here, once.  All of it inlines;
// the floating-point operations are written with the rounding intrinsics, one per operation, in the order of the oracle (these
// units build with -ffp-contract=off).  crf_update_compat_kernel does NOT use them: it carries the same statements written out,
// because with them its K x K loop was scheduled 4 % slower at K = 150 (profiles/crf_update_pieces.txt); a change here is made
// there by hand, and the tests that hold it to crf_update_kernel and crf_term_update_kernel notice a missed one.
#pragma once
#include "crf_device.h"

namespace pnp {

// A TW x TH block of pixels of one image (TW a power of two), pixels numbered pl = 0 .. TW * TH - 1 along its rows.  Slots of
// an edge tile that fall outside the image redo its last column / row (branch-free loops over the tile) and store nothing.
struct CrfTileAt {
    int x0, y0, TW, tw_shift, W, H;
    __device__ __forceinline__ int pixel_of(int pl) const {
        const int x = x0 + (pl & (TW - 1)), y = y0 + (pl >> tw_shift);
        return (y < H ? y : H - 1) * W + (x < W ? x : W - 1);
    }
    __device__ __forceinline__ bool inside(int pl) const { return x0 + (pl & (TW - 1)) < W && y0 + (pl >> tw_shift) < H; }
    // pixel_of for a caller that has tested inside(pl): no clamps
    __device__ __forceinline__ int pixel_inside(int pl) const { return (y0 + (pl >> tw_shift)) * W + x0 + (pl & (TW - 1)); }
};

// The tiles of an image, row-major
struct CrfTiles {
    int tiles_x, ntiles;
    __device__ __forceinline__ CrfTileAt at(int tl, int TW, int TH, int tw_shift, const PostDesc& im) const {
        const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
        return CrfTileAt{tx * TW, ty * TH, TW, tw_shift, im.W, im.H};
    }
};
__device__ __forceinline__ CrfTiles crf_tiles(const PostDesc& im, int TW, int TH) {
    const int tiles_x = (im.W + TW - 1) / TW, tiles_y = (im.H + TH - 1) / TH;
    return CrfTiles{tiles_x, tiles_x * tiles_y};
}
// The share [first, end) of n tiles that slice `part` of `parts` of an image takes (xcd_work)
struct CrfShare {
    int first, end;
};
__device__ __forceinline__ CrfShare crf_share(int n, int part, int parts) {
    return CrfShare{(int)((long)n * part / parts), (int)((long)n * (part + 1) / parts)};
}

// The (pixel of the tile, 16-byte chunk of its row) items of a thread: tid, tid + 256, .. in linear order, so a wave touches
// consecutive chunks whatever K4 is; the advance by 256 items carries no division
struct CrfItemWalk {
    int item, pl, c, q256, r256, K4;
    __device__ __forceinline__ CrfItemWalk(int tid, int k4) {
        K4 = k4;
        q256 = 256 / K4;
        r256 = 256 - q256 * K4;
        item = tid;
        pl = tid / K4;
        c = tid - pl * K4;
    }
    __device__ __forceinline__ void next() {
        item += 256;
        pl += q256;
        c += r256;
        if (c >= K4) {
            c -= K4;
            pl++;
        }
    }
};

// Wave roles where a lane is a pixel (the K x K products and the split softmax): WPS waves cover the TP = 32 .. 256 pixels of a
// tile, the NG = 4 / WPS waves that share a pixel set deal the labels among them (lg = 0 .. NG - 1).  A tile of 32 leaves half the
// lanes idle: they read a valid row (pxc) and write nothing (act)
struct CrfWaveRole {
    int WPS, NG, px2, lg, pxc;
    bool act;
};
__device__ __forceinline__ CrfWaveRole crf_wave_role(int TP, int tid) {
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    CrfWaveRole r;
    r.WPS = TP > 64 ? TP >> 6 : 1;
    r.NG = 4 / r.WPS;
    r.px2 = (wave % r.WPS) * 64 + lane;
    r.lg = wave / r.WPS;
    r.act = r.px2 < TP;
    r.pxc = r.act ? r.px2 : TP - 1;
    return r;
}

// The slice record of tile pixel pl (g its index in the batch) into LDS: the D1 lattice ids of its simplex, local to the image
// (lo = the image's idbase), and their barycentric weights.  One thread per pixel -- its 2 D1 words are consecutive in memory --
// so that the K4 chunk lanes of the pixel do not each fetch them
template <int D1>
__device__ __forceinline__ void crf_stage_record(const CrfLattice& L, int lo, size_t g, int pl, int* rec_o, float* rec_w) {
#pragma unroll
    for (int v = 0; v < D1; v++) {
        rec_o[pl * D1 + v] = L.offset[g * D1 + v] - lo;
        rec_w[pl * D1 + v] = L.bary[g * D1 + v];
    }
}

// The slice of one 16-byte chunk (byte offset cofs in rows of rowb bytes at Vb) in two steps, so that a kernel with two terms has
// both terms' gathers in flight before either sum: the value rows of the D1 image-local lattice ids, then
//   out = sum_v (w_v * val_v) * alpha,   v ascending, every operation rounded on its own
template <int D1>
__device__ __forceinline__ void crf_gather_rows(const char* Vb, const int* ids, uint32_t rowb, uint32_t cofs, f32x4* vv) {
#pragma unroll
    for (int v = 0; v < D1; v++) vv[v] = *reinterpret_cast<const f32x4*>(Vb + (__umul24((uint32_t)ids[v], rowb) + cofs));
}
template <int D1>
__device__ __forceinline__ f32x4 crf_slice_rows(const f32x4* vv, const float* w, float alpha) {
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < D1; v++) {
        const float wv = w[v];
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = __fadd_rn(out[i], __fmul_rn(__fmul_rn(wv, vv[v][i]), alpha));
    }
    return out;
}

// The label of tile pixel px in group grp, where labels are asked for (the last update), straight from its marginals `row` in
// LDS: first maximum, a NaN counts as maximum (np.argmax, as argmax_kernel reads them back from memory), through the LUT
__device__ __forceinline__ void crf_store_label(const CrfLabelOut& lout, int grp, int b, const CrfTileAt& at, int px, const float* row,
                                                int K) {
    if (!lout.lab[grp]) return;
    int best = 0;
    float bv = row[0];
    for (int k = 1; k < K; k++) {
        const float v = row[k];
        if (bv == bv && (v > bv || v != v)) {
            best = k;
            bv = v;
        }
    }
    if (at.inside(px)) lout.lab[grp][lout.label_off[b] + at.pixel_of(px)] = (uint8_t)lout.lut[b * lout.lut_stride + best];
}

// The rows of an LDS tile (row stride ldt) to the pixel-major rows at dst, whole 16-byte chunks, pixels inside the image only.
// STREAM: non-temporal stores (rows nobody re-reads inside the launch: st_stream).  A template argument, not a flag: given both
// stores to one address under a condition, the compiler merges them into one plain store before it knows the flag
template <bool STREAM>
__device__ __forceinline__ void crf_store_tile(const float* src, int ldt, const CrfTileAt& at, CrfItemWalk it, int TP, f32x4* dst) {
    for (; it.item < TP * it.K4; it.next()) {
        if (at.inside(it.pl)) {
            const float* r = src + it.pl * ldt + 4 * it.c;
            const f32x4 v = {r[0], r[1], r[2], r[3]};
            f32x4* const to = dst + (size_t)at.pixel_of(it.pl) * it.K4 + it.c;
            if constexpr (STREAM) st_stream(to, v);
            else *to = v;
        }
    }
}

}  // namespace pnp
