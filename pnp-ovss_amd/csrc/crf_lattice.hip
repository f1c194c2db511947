// Dense-CRF mean-field on gfx950 (replaces the pydensecrf calls at
// PnP_OVSS_0514_updated_segmentation.py:1063-1073: DenseCRF2D + addPairwiseGaussian(sxy=3,w=7) +
// addPairwiseBilateral(sxy=50,srgb=5,w=10) + inference(10)).
//
// Permutohedral lattice, built WITHOUT a hash table: every (pixel, simplex-vertex) pair emits a
// packed 64-bit lattice key; a stable segmented radix sort groups equal keys, a prefix sum over
// segment heads numbers the lattice points, blur neighbours are found by binary search in the
// sorted unique keys.  Because the sort is stable, each lattice point's contributor list is in
// ascending pixel order, so the splat is a gather that adds in exactly the order of the sequential
// CPU algorithm: results are run-to-run deterministic and bit-comparable with the oracle
// (oracle/densecrf_ref.c).  All images of a batch go through every kernel together (build kernels:
// blockIdx.y = image; iteration kernels: whole images per XCD, grids sized to what is resident).
// Nothing is reshaped into a GEMM: the iteration kernels stream 176..608-byte value rows through gathers and are
// bound by memory latency x occupancy and by vector-memory issue, so they are written around
// their dependent-load chains: contributor / neighbour / slice records, requests of the next item behind the
// gathers of the current one, results stored one item later.
//
// This unit: the lattice build (keys, embed, heads, neighbour search, renumbering, contributor segments) and the normaliser.
// The mean-field iteration kernels are in crf_meanfield.hip, the reverse mode in crf_grad.hip; what the three share: crf_device.h.
#include "crf_device.h"

namespace pnp {

template <int D> struct KeyPack;
template <> struct KeyPack<2> { static constexpr int BITS = 16; };
template <> struct KeyPack<5> { static constexpr int BITS = 11; };
// The image index of the batch sits above the coordinate bits (bit IMG_SHIFT..).  It is NOT sorted on: the entries arrive
// image by image, so crf_build_lattice runs sort.hip's stable radix sort segmented by image over the coordinate bits alone;
// the image bits stay in the keys for what reads them afterwards (mark_heads: a run never spans two images; the neighbour
// search compares whole keys).  5 x 11 + 6 bits <= 61: at most 64 images per prepared batch.
constexpr int IMG_SHIFT = 55;
constexpr int IMG_BITS = 6;
// Keys of the feature path (lattice_embed_features_kernel, D = 1 .. 6 caller-supplied axes): WITHOUT image bits -- mark_heads
// takes the image boundaries from the descriptors and the neighbour search stays inside idbase[b] .. idbase[b + 1], so all 64
// bits are coordinates: 16, 16, 16, 16, 12, 10 per coordinate (D = 6: |coordinate| < 2^9 - 7 = 505; the 9 bits that 55 / 6
// leave reach 249, too few for xy / 50, rgb / 5 and one more channel on a 375 x 500 image)
template <int D> struct FeatKey { static constexpr int BITS = 64 / D < 16 ? 64 / D : 16; };
// |elevated coordinate| the feature path accepts whatever the key holds: rem0 and the keys pass through int16 as in densecrf
constexpr float CRF_FEAT_ELEV_LIMIT = 32000.f;

template <int D, int BITS = KeyPack<D>::BITS>
__device__ __forceinline__ uint64_t pack_key(const int* c) {
    uint64_t k = 0;
#pragma unroll
    for (int i = 0; i < D; i++) k = (k << BITS) | (uint64_t)((c[i] + (1 << (BITS - 1))) & ((1 << BITS) - 1));
    return k;
}
template <int D, int BITS = KeyPack<D>::BITS>
__device__ __forceinline__ void unpack_key(uint64_t k, int* c) {
#pragma unroll
    for (int i = D - 1; i >= 0; i--) {
        c[i] = (int)(k & ((1 << BITS) - 1)) - (1 << (BITS - 1));      // image bits above D*BITS are ignored
        k >>= BITS;
    }
}

// ------------------------------------------------------------------------------------------
// Per pixel: features -> elevate -> nearest remainder-0 point -> rank -> barycentric -> d+1 keys.
// Mirrors oracle/densecrf_ref.c::lattice_init statement by statement (fp contraction is off for
// this translation unit) so barycentric weights and keys are bit-identical.
template <int D>
__global__ void lattice_embed_kernel(const PostDesc* __restrict__ imgs, const uint8_t* __restrict__ rgb, float sx, float sy, float sr,
                                     float sg, float sb, float* __restrict__ bary, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                     int* __restrict__ range_err) {
    const int b = blockIdx.y;
    const PostDesc im = imgs[b];
    const int n = im.H * im.W;
    float scale_factor[D];
    {
        const float inv_std_dev = (float)(sqrt(2.0 / 3.0) * (D + 1));
#pragma unroll
        for (int i = 0; i < D; i++) scale_factor[i] = (float)(1.0 / sqrt((double)((i + 2) * (i + 1))) * inv_std_dev);
    }
    for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < n; pix += gridDim.x * blockDim.x) {
        const int y = pix / im.W, x = pix - y * im.W;
        float f[D];
        f[0] = __fdiv_rn((float)x, sx);
        f[1] = __fdiv_rn((float)y, sy);
        if constexpr (D == 5) {
            const uint8_t* c = rgb + ((size_t)im.pix0 + pix) * 3;
            f[2] = __fdiv_rn((float)c[0], sr);
            f[3] = __fdiv_rn((float)c[1], sg);
            f[4] = __fdiv_rn((float)c[2], sb);
        }
        float elevated[D + 1], rem0[D + 1], barycentric[D + 2];
        int rank[D + 1];
        float sm = 0.f;
#pragma unroll
        for (int j = D; j > 0; j--) {
            const float cf = __fmul_rn(f[j - 1], scale_factor[j - 1]);
            elevated[j] = __fsub_rn(sm, __fmul_rn((float)j, cf));
            sm = __fadd_rn(sm, cf);
        }
        elevated[0] = sm;
        const float down_factor = 1.0f / (D + 1);
        const float up_factor = (float)(D + 1);
        int sum = 0;
#pragma unroll
        for (int i = 0; i <= D; i++) {
            const float v = __fmul_rn(down_factor, elevated[i]);
            const float up = __fmul_rn(ceilf(v), up_factor);
            const float down = __fmul_rn(floorf(v), up_factor);
            int rd2;
            if (__fsub_rn(up, elevated[i]) < __fsub_rn(elevated[i], down)) rd2 = (int)(short)up;
            else rd2 = (int)(short)down;
            rem0[i] = (float)rd2;
            sum = (int)__fadd_rn((float)sum, __fmul_rn((float)rd2, down_factor));
        }
#pragma unroll
        for (int i = 0; i <= D; i++) rank[i] = 0;
#pragma unroll
        for (int i = 0; i < D; i++) {
            const double di = (double)__fsub_rn(elevated[i], rem0[i]);
#pragma unroll
            for (int j = i + 1; j <= D; j++) {
                if (di < (double)__fsub_rn(elevated[j], rem0[j])) rank[i]++;
                else rank[j]++;
            }
        }
#pragma unroll
        for (int i = 0; i <= D; i++) {
            rank[i] += sum;
            if (rank[i] < 0) {
                rank[i] += D + 1;
                rem0[i] = __fadd_rn(rem0[i], (float)(D + 1));
            } else if (rank[i] > D) {
                rank[i] -= D + 1;
                rem0[i] = __fsub_rn(rem0[i], (float)(D + 1));
            }
        }
#pragma unroll
        for (int i = 0; i <= D + 1; i++) barycentric[i] = 0.f;
#pragma unroll
        for (int i = 0; i <= D; i++) {
            const float v = __fmul_rn(__fsub_rn(elevated[i], rem0[i]), down_factor);
            // barycentric[D - rank[i]] += v ; barycentric[D - rank[i] + 1] -= v   (static indexing)
#pragma unroll
            for (int s = 0; s <= D + 1; s++) {
                if (s == D - rank[i]) barycentric[s] = __fadd_rn(barycentric[s], v);
                if (s == D - rank[i] + 1) barycentric[s] = __fsub_rn(barycentric[s], v);
            }
        }
        barycentric[0] = __fadd_rn(barycentric[0], __fadd_rn(1.0f, barycentric[D + 1]));

        const size_t e0 = (size_t)(im.pix0 + pix) * (D + 1);
#pragma unroll
        for (int rem = 0; rem <= D; rem++) {
            int key[D];
            bool bad = false;
#pragma unroll
            for (int i = 0; i < D; i++) {
                // canonical[rem][rank[i]] = rem if rank[i] <= D - rem else rem - (D+1)
                const int canon = (rank[i] <= D - rem) ? rem : rem - (D + 1);
                key[i] = (int)(short)(rem0[i] + (float)canon);
                bad |= (key[i] <= -(1 << (KeyPack<D>::BITS - 1)) + D + 1) || (key[i] >= (1 << (KeyPack<D>::BITS - 1)) - D - 1);
            }
            if (bad) atomicExch(range_err, 1);
            keys[e0 + rem] = pack_key<D>(key) | ((uint64_t)b << IMG_SHIFT);
            vals[e0 + rem] = (uint32_t)(e0 + rem);
            bary[e0 + rem] = barycentric[rem];
        }
    }
}

// The same embedding on D = 1 .. 6 features the caller brings (pnp_crf_set_batch_terms): image b's block of `feat` is D planes of
// H * W floats at float offset pix0 * D, already divided by their widths, so a wave reads 256 consecutive bytes of every plane.
// From `elevated` on these are lattice_embed_kernel's statements (tests: xy and xy+rgb features give its lattices bit for bit)
// with the feature path's key (FeatKey: no image bits) and one more reason to raise the range flag: a non-finite feature, or
// an elevated coordinate beyond CRF_FEAT_ELEV_LIMIT, where rem0 and the keys would wrap in their int16 casts and could land
// back inside the key's range.  (The statements are repeated, not shared through a function: with the body factored out
// lattice_embed_kernel compiled to other instructions, and the two-term path keeps the ones it had.)
template <int D>
__global__ void lattice_embed_features_kernel(const PostDesc* __restrict__ imgs, const float* __restrict__ feat, float* __restrict__ bary,
                                              uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, int* __restrict__ range_err) {
    constexpr int BITS = FeatKey<D>::BITS;
    const int b = blockIdx.y;
    const PostDesc im = imgs[b];
    const int n = im.H * im.W;
    const float* const fb = feat + (size_t)im.pix0 * D;
    float scale_factor[D];
    {
        const float inv_std_dev = (float)(sqrt(2.0 / 3.0) * (D + 1));
#pragma unroll
        for (int i = 0; i < D; i++) scale_factor[i] = (float)(1.0 / sqrt((double)((i + 2) * (i + 1))) * inv_std_dev);
    }
    for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < n; pix += gridDim.x * blockDim.x) {
        float f[D];
#pragma unroll
        for (int i = 0; i < D; i++) f[i] = ld_stream(fb + (size_t)i * n + pix);
        const size_t e0 = (size_t)(im.pix0 + pix) * (D + 1);
        float elevated[D + 1], rem0[D + 1], barycentric[D + 2];
        int rank[D + 1];
        float sm = 0.f;
#pragma unroll
        for (int j = D; j > 0; j--) {
            const float cf = __fmul_rn(f[j - 1], scale_factor[j - 1]);
            elevated[j] = __fsub_rn(sm, __fmul_rn((float)j, cf));
            sm = __fadd_rn(sm, cf);
        }
        elevated[0] = sm;
        const float down_factor = 1.0f / (D + 1);
        const float up_factor = (float)(D + 1);
        int sum = 0;
#pragma unroll
        for (int i = 0; i <= D; i++) {
            const float v = __fmul_rn(down_factor, elevated[i]);
            const float up = __fmul_rn(ceilf(v), up_factor);
            const float down = __fmul_rn(floorf(v), up_factor);
            int rd2;
            if (__fsub_rn(up, elevated[i]) < __fsub_rn(elevated[i], down)) rd2 = (int)(short)up;
            else rd2 = (int)(short)down;
            rem0[i] = (float)rd2;
            sum = (int)__fadd_rn((float)sum, __fmul_rn((float)rd2, down_factor));
        }
#pragma unroll
        for (int i = 0; i <= D; i++) rank[i] = 0;
#pragma unroll
        for (int i = 0; i < D; i++) {
            const double di = (double)__fsub_rn(elevated[i], rem0[i]);
#pragma unroll
            for (int j = i + 1; j <= D; j++) {
                if (di < (double)__fsub_rn(elevated[j], rem0[j])) rank[i]++;
                else rank[j]++;
            }
        }
#pragma unroll
        for (int i = 0; i <= D; i++) {
            rank[i] += sum;
            if (rank[i] < 0) {
                rank[i] += D + 1;
                rem0[i] = __fadd_rn(rem0[i], (float)(D + 1));
            } else if (rank[i] > D) {
                rank[i] -= D + 1;
                rem0[i] = __fsub_rn(rem0[i], (float)(D + 1));
            }
        }
#pragma unroll
        for (int i = 0; i <= D + 1; i++) barycentric[i] = 0.f;
#pragma unroll
        for (int i = 0; i <= D; i++) {
            const float v = __fmul_rn(__fsub_rn(elevated[i], rem0[i]), down_factor);
            // barycentric[D - rank[i]] += v ; barycentric[D - rank[i] + 1] -= v   (static indexing)
#pragma unroll
            for (int s = 0; s <= D + 1; s++) {
                if (s == D - rank[i]) barycentric[s] = __fadd_rn(barycentric[s], v);
                if (s == D - rank[i] + 1) barycentric[s] = __fsub_rn(barycentric[s], v);
            }
        }
        barycentric[0] = __fadd_rn(barycentric[0], __fadd_rn(1.0f, barycentric[D + 1]));

        bool wild = false;                                  // beyond what the int16 casts below hold, or not finite
        #pragma unroll
        for (int i = 0; i <= D; i++) wild |= !(fabsf(elevated[i]) < CRF_FEAT_ELEV_LIMIT);          // (a NaN compares false)
#pragma unroll
        for (int rem = 0; rem <= D; rem++) {
            int key[D];
            bool bad = wild;
#pragma unroll
            for (int i = 0; i < D; i++) {
                // canonical[rem][rank[i]] = rem if rank[i] <= D - rem else rem - (D+1)
                const int canon = (rank[i] <= D - rem) ? rem : rem - (D + 1);
                key[i] = (int)(short)(rem0[i] + (float)canon);
                bad |= (key[i] <= -(1 << (BITS - 1)) + D + 1) || (key[i] >= (1 << (BITS - 1)) - D - 1);
            }
            if (bad) atomicExch(range_err, 1);
            keys[e0 + rem] = pack_key<D, BITS>(key);
            vals[e0 + rem] = (uint32_t)(e0 + rem);
            bary[e0 + rem] = barycentric[rem];
        }
    }
}

// head[i] = 1 where sorted entry i starts a new lattice point (first entry of the image or new key)
__global__ void mark_heads_kernel(const uint64_t* __restrict__ keys, const PostDesc* __restrict__ imgs, int D1,
                                  int* __restrict__ head) {
    const int b = blockIdx.y;
    const PostDesc im = imgs[b];
    const size_t e0 = (size_t)im.pix0 * D1, n = (size_t)im.H * im.W * D1;
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        head[e0 + i] = (i == 0 || keys[e0 + i] != keys[e0 + i - 1]) ? 1 : 0;
}

// ids: inclusive scan of head.  offset[pv] = lattice id; seg_start[id] = first sorted entry;
// ukeys[id] = key; idbase[b] = id of the image's first entry; idbase[B] = seg_start[M] sentinel.
__global__ void scatter_ids_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                   const int* __restrict__ head, const int* __restrict__ incl, const PostDesc* __restrict__ imgs,
                                   int D1, int B, size_t ent_total, int* __restrict__ offset, int* __restrict__ seg_start,
                                   uint64_t* __restrict__ ukeys, int* __restrict__ idbase) {
    const int b = blockIdx.y;
    const PostDesc im = imgs[b];
    const size_t e0 = (size_t)im.pix0 * D1, n = (size_t)im.H * im.W * D1;
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t g = e0 + i;
        const int id = incl[g] - 1;
        offset[vals[g]] = id;
        if (head[g]) {
            seg_start[id] = (int)g;
            ukeys[id] = keys[g];
        }
        if (i == 0) idbase[b] = id;
        if (b == B - 1 && i == n - 1) {
            idbase[B] = id + 1;
            seg_start[id + 1] = (int)ent_total;
        }
    }
}

// blur neighbours along each of the d+1 lattice axes: n1 = key - 1 (coord j: + d), n2 = key + 1 (coord j: - d).
// A neighbour's key is the point's key plus a constant of the axis (the fields are positional digits and a key whose neighbour
// would leave a field's range is flagged absent), so along the sorted unique keys of an image the neighbour positions are
// monotone: a thread takes a RUN of consecutive points of one axis, finds the first neighbour by binary search (17 dependent
// loads at 100 k points) and the others by galloping from the previous position (2-3 loads).
constexpr int kNbrRun = 8;
__device__ __forceinline__ int lower_bound_from(const uint64_t* __restrict__ ukeys, int from, int hi, uint64_t key) {
    // first position in [from, hi) whose key is >= key, given that every position before `from` holds a smaller key
    int l = from, step = 1;
    while (l + step <= hi && ukeys[l + step - 1] < key) {      // gallop: the answer is beyond l + step - 1
        l += step;
        step <<= 1;
    }
    int h = l + step - 1 < hi ? l + step - 1 : hi;             // answer in [l, h]
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (ukeys[mid] < key) l = mid + 1;
        else h = mid;
    }
    return l;
}
// IMG: the keys carry the image index above their coordinates (the xy / xy+rgb path; the feature path's do not)
template <int D, int BITS = KeyPack<D>::BITS, bool IMG = true>
__global__ void neighbors_kernel(const uint64_t* __restrict__ ukeys, const int* __restrict__ idbase, size_t cap,
                                 int* __restrict__ n1, int* __restrict__ n2) {
    const int b = blockIdx.y;
    const uint64_t image = IMG ? (uint64_t)b << IMG_SHIFT : 0;
    const int lo = idbase[b], hi = idbase[b + 1];
    const int nruns = (hi - lo + kNbrRun - 1) / kNbrRun;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nruns * (D + 1); t += gridDim.x * blockDim.x) {
        const int run = t / (D + 1), j = t % (D + 1);
        const int id0 = lo + run * kNbrRun, id1 = id0 + kNbrRun < hi ? id0 + kNbrRun : hi;
        int p1 = lo, p2 = lo;                                   // positions reached so far (nothing before them can match)
        bool first1 = true, first2 = true;
        for (int id = id0; id < id1; id++) {
            int c[D], a[D], d2[D];
            unpack_key<D, BITS>(ukeys[id], c);
#pragma unroll
            for (int k = 0; k < D; k++) {
                a[k] = c[k] - 1;
                d2[k] = c[k] + 1;
            }
#pragma unroll
            for (int k = 0; k < D; k++)
                if (k == j) {
                    a[k] = c[k] + D;
                    d2[k] = c[k] - D;
                }
            int r1 = -1, r2 = -1;
            bool in1 = true, in2 = true;
#pragma unroll
            for (int k = 0; k < D; k++) {
                in1 &= (a[k] >= -(1 << (BITS - 1)) && a[k] < (1 << (BITS - 1)));
                in2 &= (d2[k] >= -(1 << (BITS - 1)) && d2[k] < (1 << (BITS - 1)));
            }
            if (in1) {
                const uint64_t k1 = pack_key<D, BITS>(a) | image;
                int l;
                if (first1) {                                   // binary search inside this image's sorted unique keys [lo, hi)
                    int ll = lo, h = hi;
                    while (ll < h) {
                        const int mid = (ll + h) >> 1;
                        if (ukeys[mid] < k1) ll = mid + 1;
                        else h = mid;
                    }
                    l = ll;
                    first1 = false;
                } else {
                    l = lower_bound_from(ukeys, p1, hi, k1);
                }
                p1 = l;
                if (l < hi && ukeys[l] == k1) r1 = l;
            }
            if (in2) {
                const uint64_t k2 = pack_key<D, BITS>(d2) | image;
                int l;
                if (first2) {
                    int ll = lo, h = hi;
                    while (ll < h) {
                        const int mid = (ll + h) >> 1;
                        if (ukeys[mid] < k2) ll = mid + 1;
                        else h = mid;
                    }
                    l = ll;
                    first2 = false;
                } else {
                    l = lower_bound_from(ukeys, p2, hi, k2);
                }
                p2 = l;
                if (l < hi && ukeys[l] == k2) r2 = l;
            }
            n1[(size_t)j * cap + id] = r1;
            n2[(size_t)j * cap + id] = r2;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Scalar (K = 1) lattice pass used once per batch for the normaliser: norm = 1/sqrt(L(1) + 1e-20).

__global__ void crf_splat1_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs, float* __restrict__ val) {
    const int b = blockIdx.y;
    const int lo = L.idbase[b], hi = L.idbase[b + 1];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < hi - lo; t += gridDim.x * blockDim.x) {
        const int id = lo + t;
        const int e0 = L.seg_lo[id], e1 = L.seg_hi[id];
        float acc = 0.f;
        for (int e = e0; e < e1; e++) acc = __fadd_rn(acc, L.bary[L.vals[e]]);
        val[id] = acc;
    }
}

__global__ void crf_blur1_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs, const float* __restrict__ src,
                                 float* __restrict__ dst, int axis) {
    const int b = blockIdx.y;
    const int lo = L.idbase[b], hi = L.idbase[b + 1];
    const int* n1 = L.n1 + (size_t)axis * L.cap;
    const int* n2 = L.n2 + (size_t)axis * L.cap;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < hi - lo; t += gridDim.x * blockDim.x) {
        const int id = lo + t;
        const int a = n1[id], c = n2[id];
        const float va = a >= 0 ? src[a] : 0.f;
        const float vc = c >= 0 ? src[c] : 0.f;
        dst[id] = crf_axis(src[id], va, vc);
    }
}

__global__ void crf_norm_kernel(const CrfLattice L, const PostDesc* __restrict__ imgs, const float* __restrict__ val,
                                float* __restrict__ norm_out, float alpha) {
    const int b = blockIdx.y;
    const PostDesc im = imgs[b];
    const int n = im.H * im.W;
    for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < n; pix += gridDim.x * blockDim.x) {
        const size_t pv0 = (size_t)(im.pix0 + pix) * L.D1;
        float out = 0.f;
        for (int v = 0; v < L.D1; v++)
            out = __fadd_rn(out, __fmul_rn(__fmul_rn(L.bary[pv0 + v], val[L.offset[pv0 + v]]), alpha));
        norm_out[im.pix0 + pix] = (float)(1.0 / sqrt((double)out + 1e-20));
    }
}

// contributor records get the normaliser of their pixel (the splat multiplies Q * norm before the barycentric weight)
__global__ void entry_norm_kernel(CrfEntry* __restrict__ ent, size_t n, const float* __restrict__ norm) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        ent[i].nr = norm[ent[i].pixel];
}

// ---- spatial renumbering.  The key sort numbers lattice points in (colour-major) key order; the
// iteration kernels are gather-bound, so the points of each image are renumbered by the position of their
// FIRST contributor pixel along a Z-order curve over the image: contributors, simplex vertices of neighbouring
// pixels and blur neighbours (all within about one spatial cell, sxy pixels, in both directions) then sit in
// nearby value rows and the gathers hit L2.  Against row-major pixel order: the same at 0.9 lattice points per pixel,
// 7 % less mean-field time at 3.6.  Lattice ids are internal: results do not depend on them.
__device__ __forceinline__ uint32_t morton_spread(uint32_t v) {          // 16 bits -> every second bit
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}
// sort key of a lattice point: (image | position of its first contributor pixel along a Z-order curve over the image | vertex)
__global__ void first_contrib_kernel(const uint32_t* __restrict__ vals, const int* __restrict__ seg_start, int M,
                                     const PostDesc* __restrict__ imgs, const int* __restrict__ idbase, int B, int D1,
                                     uint64_t* __restrict__ fkey, uint32_t* __restrict__ fid) {
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < M; id += gridDim.x * blockDim.x) {
        const uint32_t pv = vals[seg_start[id]];
        int lo = 0, hi = B;                                  // image of the point: idbase[lo] <= id < idbase[lo + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (idbase[mid] <= id) lo = mid;
            else hi = mid;
        }
        const uint32_t pixel = pv / (uint32_t)D1, v = pv - pixel * (uint32_t)D1;
        const uint32_t local = pixel - (uint32_t)imgs[lo].pix0;
        const uint32_t W = (uint32_t)imgs[lo].W, y = local / W, x = local - y * W;
        const uint64_t pos = (uint64_t)morton_spread(x) | ((uint64_t)morton_spread(y) << 1);
        fkey[id] = ((uint64_t)lo << 40) | (pos << 3) | v;
        fid[id] = (uint32_t)id;
    }
}
__global__ void rank_kernel(const uint32_t* __restrict__ sorted_id, int M, int* __restrict__ rank) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) rank[sorted_id[i]] = i;
}
__global__ void renumber_points_kernel(const int* __restrict__ rank, const int* __restrict__ seg_start,
                                       const int* __restrict__ n1k, const int* __restrict__ n2k, size_t cap, int M, int D1,
                                       int* __restrict__ seg_lo, int* __restrict__ seg_hi, int* __restrict__ n1,
                                       int* __restrict__ n2) {
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < M; id += gridDim.x * blockDim.x) {
        const int nid = rank[id];
        seg_lo[nid] = seg_start[id];
        seg_hi[nid] = seg_start[id + 1];
        for (int j = 0; j < D1; j++) {
            const int a = n1k[(size_t)j * cap + id], b = n2k[(size_t)j * cap + id];
            n1[(size_t)j * cap + nid] = a >= 0 ? rank[a] : -1;
            n2[(size_t)j * cap + nid] = b >= 0 ? rank[b] : -1;
        }
    }
}
__global__ void renumber_entries_kernel(const int* __restrict__ rank, size_t n, int* __restrict__ offset) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        offset[i] = rank[offset[i]];
}

// ---- neighbour records of the two-axis blur: for axis pair (2p, 2p+1) the point's neighbours along axis 2p (ia, id), along
// axis 2p+1 (pa, pd) and the axis-2p neighbours of those two (aa, ad, da, dd), as image-local ids (-1 = absent)
__global__ void nbr8_kernel(const int* __restrict__ n1, const int* __restrict__ n2, size_t cap, const int* __restrict__ idbase,
                            int npairs, CrfNbr8* __restrict__ out) {
    const int b = blockIdx.y;
    const int lo = idbase[b], hi = idbase[b + 1];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < (hi - lo) * npairs; t += gridDim.x * blockDim.x) {
        const int id = lo + t / npairs, pr = t % npairs;
        const int* n1a = n1 + (size_t)(2 * pr) * cap;
        const int* n2a = n2 + (size_t)(2 * pr) * cap;
        const int* n1b = n1 + (size_t)(2 * pr + 1) * cap;
        const int* n2b = n2 + (size_t)(2 * pr + 1) * cap;
        const int pa = n1b[id], pd = n2b[id];
        CrfNbr8 r;
        r.ia = n1a[id];
        r.id = n2a[id];
        r.pa = pa;
        r.pd = pd;
        r.aa = pa >= 0 ? n1a[pa] : -1;
        r.ad = pa >= 0 ? n2a[pa] : -1;
        r.da = pd >= 0 ? n1a[pd] : -1;
        r.dd = pd >= 0 ? n2a[pd] : -1;
        int* q = &r.ia;
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = q[k] >= 0 ? q[k] - lo : -1;
        out[(size_t)pr * cap + id] = r;
    }
}

// ---- contributor lists in lattice-id order.  The key sort leaves each point's contributor segment where its KEY
// sorted; after the spatial renumbering consecutive lattice ids own segments scattered over the whole list.  The
// segments are moved (each keeps its ascending-pixel order) so that id order = list order: the splat then walks the
// list front to back, and a range of lattice points is a contiguous range of contributors.
__global__ void seg_len_kernel(const int* __restrict__ seg_lo, const int* __restrict__ seg_hi, int M, int* __restrict__ len) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) len[i] = seg_hi[i] - seg_lo[i];
}
__global__ void move_segments_kernel(const uint32_t* __restrict__ vals, const int* __restrict__ new_start, int M, int D1,
                                     const float* __restrict__ bary, int* __restrict__ seg_lo, int* __restrict__ seg_hi,
                                     uint32_t* __restrict__ vals2, CrfEntry* __restrict__ ent) {
    // eight lanes per lattice point: the entries of a segment are copied side by side (one thread per point walked its
    // segment alone: 16-byte records at scattered addresses, 0.49 ms per build)
    const long nthr = (long)gridDim.x * blockDim.x;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < (long)M * 8; t += nthr) {
        const int i = (int)(t >> 3), j0 = (int)(t & 7);
        const int a = seg_lo[i], n = seg_hi[i] - a, d = new_start[i];
        for (int j = j0; j < n; j += 8) {
            const uint32_t pv = vals[a + j];
            vals2[d + j] = pv;
            ent[d + j] = CrfEntry{pv / (uint32_t)D1, bary[pv], 0.f, 0u};  // the splat's contributor record (nr: crf_lattice_norm)
        }
    }
}
// (the segment bounds are rewritten once every lane group has read the old ones: separate launch)
__global__ void set_segments_kernel(const int* __restrict__ new_start, int M, int* __restrict__ seg_lo, int* __restrict__ seg_hi) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const int n = seg_hi[i] - seg_lo[i], d = new_start[i];
        seg_lo[i] = d;
        seg_hi[i] = d + n;
    }
}

// ------------------------------------------------------------------------------------------ host
size_t crf_sort_temp_bytes(size_t max_entries) { return sort_temp_bytes(max_entries) + 256; }

// Build one lattice for images [0,B).  d_feat null: D = 2 (Gaussian x/sx, y/sy) or D = 5 (bilateral x/sx, y/sy, r/sr, g/sg, b/sb)
// from pixel positions and d_rgb, sxy = (sx, sy), srgb = (sr, sg, sb), one width per feature axis.  d_feat: D = 1 .. 6 feature
// planes of the caller's (lattice_embed_features_kernel; keys without image bits).  The scratch arrays and the roles each of
// them takes in turn: CrfBuildScratch (kernels.h).
static int build_lattice(int D, const CrfLattice& L, const PostDesc* d_imgs, const PostDesc* h_imgs, const uint8_t* d_rgb, const float sxy[2],
                         const float srgb[3], const float* d_feat, int B, size_t ent_total, int max_pixels, const CrfBuildScratch& sc,
                         int* h_range_err, int* h_points, hipStream_t s) {
    const int nb = (max_pixels + 255) / 256 < 512 ? (max_pixels + 255) / 256 : 512;
    int coord_bits = 0;
    if (d_feat) {
        const int r = crf_dispatch<1, 6>(D, [&](auto d) {
            constexpr int D_ = decltype(d)::value;
            hipLaunchKernelGGL((lattice_embed_features_kernel<D_>), dim3(nb, B), dim3(256), 0, s, d_imgs, d_feat, L.bary, sc.keys_a, sc.vals_a,
                               sc.range_err);
            coord_bits = D_ * FeatKey<D_>::BITS;
            return PNP_OK;
        });
        if (r != PNP_OK) return r;
    } else if (D == 2)
        hipLaunchKernelGGL((lattice_embed_kernel<2>), dim3(nb, B), dim3(256), 0, s, d_imgs, d_rgb, sxy[0], sxy[1], srgb[0], srgb[1], srgb[2], L.bary, sc.keys_a, sc.vals_a, sc.range_err);
    else if (D == 5)
        hipLaunchKernelGGL((lattice_embed_kernel<5>), dim3(nb, B), dim3(256), 0, s, d_imgs, d_rgb, sxy[0], sxy[1], srgb[0], srgb[1], srgb[2], L.bary, sc.keys_a, sc.vals_a, sc.range_err);
    else
        return PNP_ERR_ARG;
    if (B > (1 << IMG_BITS)) return PNP_ERR_ARG;
    // bits actually populated: coordinates (D * BITS, low) + image index (IMG_SHIFT..)
    // stable sort by (image, coordinates).  The entries of image b are the run [pix0 * (D+1), (pix0 + H W) * (D+1)) on entry, so
    // the sort is segmented by image over the coordinate bits [0, D * BITS) alone (sort.hip; the image bits at IMG_SHIFT stay in
    // the keys for the kernels below; the inputs sc.keys_a / sc.vals_a are scratch from here on)
    if (!d_feat) coord_bits = D == 2 ? 2 * KeyPack<2>::BITS : 5 * KeyPack<5>::BITS;
    size_t seg_off[(1 << IMG_BITS) + 1];
    for (int b = 0; b < B; b++) {
        seg_off[b] = (size_t)h_imgs[b].pix0 * (D + 1);
        if (b && seg_off[b] != seg_off[b - 1] + (size_t)h_imgs[b - 1].H * h_imgs[b - 1].W * (D + 1)) return PNP_ERR_ARG;
    }
    seg_off[B] = ent_total;
    if (B < 1 || seg_off[0] != 0 || seg_off[B - 1] + (size_t)h_imgs[B - 1].H * h_imgs[B - 1].W * (D + 1) != ent_total) return PNP_ERR_ARG;
    {
        const int r = radix_sort_pairs(sc.keys_a, sc.keys_b, sc.vals_a, L.vals, ent_total, 0, coord_bits, seg_off, B, sc.temp, sc.temp_bytes, s);
        if (r != PNP_OK) return r;
    }
    const int nbe = 1024;
    hipLaunchKernelGGL(mark_heads_kernel, dim3(nbe, B), dim3(256), 0, s, sc.keys_b, d_imgs, D + 1, sc.head);
    if (const int r = device_scan_i32(sc.head, sc.incl, ent_total, true, sc.temp, sc.temp_bytes, s); r != PNP_OK) return r;
    hipLaunchKernelGGL(scatter_ids_kernel, dim3(nbe, B), dim3(256), 0, s, sc.keys_b, L.vals, sc.head, sc.incl, d_imgs, D + 1, B,
                       ent_total, L.offset, L.seg_start, L.ukeys, L.idbase);
    if (d_feat)
        (void)crf_dispatch<1, 6>(D, [&](auto d) {                // (D is in range: the embed above)
            constexpr int D_ = decltype(d)::value;
            hipLaunchKernelGGL((neighbors_kernel<D_, FeatKey<D_>::BITS, false>), dim3(nbe, B), dim3(256), 0, s, L.ukeys, L.idbase, L.cap, sc.n1k,
                               sc.n2k);
            return PNP_OK;
        });
    else if (D == 2)
        hipLaunchKernelGGL((neighbors_kernel<2>), dim3(nbe, B), dim3(256), 0, s, L.ukeys, L.idbase, L.cap, sc.n1k, sc.n2k);
    else
        hipLaunchKernelGGL((neighbors_kernel<5>), dim3(nbe, B), dim3(256), 0, s, L.ukeys, L.idbase, L.cap, sc.n1k, sc.n2k);
    // spatial renumbering (needs the lattice size on the host: one small read-back per build)
    int M = 0;
    int h_idbase[(1 << IMG_BITS) + 1];                    // first lattice id of every image (the second sort's segments)
    // (the key-range flag of the embed kernel rides on the same synchronisation)
    int err = 0;
    if (hipMemcpyAsync(h_idbase, L.idbase, sizeof(int) * (B + 1), hipMemcpyDeviceToHost, s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemcpyAsync(&err, sc.range_err, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return PNP_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return PNP_ERR_HIP;
    M = h_idbase[B];
    if (err && h_range_err) *h_range_err = 1;
    if (M <= 0 || (size_t)M > ent_total) return PNP_ERR_STATE;
    if (h_points) *h_points = M;                          // lattice points of the batch (bench.py: lattice term of the byte model)
    uint64_t* fkey = sc.keys_a;
    uint64_t* skey = sc.keys_b;
    uint32_t* fid = sc.vals_a;
    uint32_t* sid = reinterpret_cast<uint32_t*>(sc.incl);
    int* rank = sc.head;
    hipLaunchKernelGGL(first_contrib_kernel, dim3(1024), dim3(256), 0, s, L.vals, L.seg_start, M, d_imgs, L.idbase, B, D + 1, fkey, fid);
    {   // lattice points are numbered image by image: segmented by image over (Z-order position, vertex) = bits [0, 40)
        size_t seg2[(1 << IMG_BITS) + 1];
        for (int b = 0; b <= B; b++) seg2[b] = (size_t)h_idbase[b];
        if (const int r = radix_sort_pairs(fkey, skey, fid, sid, (size_t)M, 0, 40, seg2, B, sc.temp, sc.temp_bytes, s); r != PNP_OK) return r;
    }
    hipLaunchKernelGGL(rank_kernel, dim3(1024), dim3(256), 0, s, sid, M, rank);
    hipLaunchKernelGGL(renumber_points_kernel, dim3(1024), dim3(256), 0, s, rank, L.seg_start, sc.n1k, sc.n2k, L.cap, M, D + 1,
                       L.seg_lo, L.seg_hi, L.n1, L.n2);
    hipLaunchKernelGGL(renumber_entries_kernel, dim3(2048), dim3(256), 0, s, rank, ent_total, L.offset);
    hipLaunchKernelGGL(nbr8_kernel, dim3(256, B), dim3(256), 0, s, L.n1, L.n2, L.cap, L.idbase, (D + 1) / 2, L.nbr8);
    // contributor segments into lattice-id order
    int* len = reinterpret_cast<int*>(sc.keys_a);
    uint32_t* vals2 = reinterpret_cast<uint32_t*>(sc.keys_b);
    hipLaunchKernelGGL(seg_len_kernel, dim3(1024), dim3(256), 0, s, L.seg_lo, L.seg_hi, M, len);
    if (const int r = device_scan_i32(len, sc.incl, (size_t)M, false, sc.temp, sc.temp_bytes, s); r != PNP_OK) return r;
    hipLaunchKernelGGL(move_segments_kernel, dim3(4096), dim3(256), 0, s, L.vals, sc.incl, M, D + 1, L.bary, L.seg_lo, L.seg_hi, vals2, L.ent);
    hipLaunchKernelGGL(set_segments_kernel, dim3(1024), dim3(256), 0, s, sc.incl, M, L.seg_lo, L.seg_hi);
    if (hipMemcpyAsync(L.vals, vals2, ent_total * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) return PNP_ERR_HIP;
    return ok();
}

int crf_build_lattice(int D, const CrfLattice& L, const PostDesc* d_imgs, const PostDesc* h_imgs, const uint8_t* d_rgb, const float sxy[2],
                      const float srgb[3], int B, size_t ent_total, int max_pixels, const CrfBuildScratch& sc, int* h_range_err, int* h_points,
                      hipStream_t s) {
    return build_lattice(D, L, d_imgs, h_imgs, d_rgb, sxy, srgb, nullptr, B, ent_total, max_pixels, sc, h_range_err, h_points, s);
}

int crf_build_lattice_features(int D, const CrfLattice& L, const PostDesc* d_imgs, const PostDesc* h_imgs, const float* d_feat, int B,
                               size_t ent_total, int max_pixels, const CrfBuildScratch& sc, int* h_range_err, int* h_points, hipStream_t s) {
    if (!d_feat) return PNP_ERR_ARG;
    return build_lattice(D, L, d_imgs, h_imgs, nullptr, nullptr, nullptr, d_feat, B, ent_total, max_pixels, sc, h_range_err, h_points, s);
}

int crf_feature_key_limit(int D) {
    const int bits = 64 / D < 16 ? 64 / D : 16;
    const int by_key = (1 << (bits - 1)) - D - 1;
    return by_key < (int)CRF_FEAT_ELEV_LIMIT ? by_key : (int)CRF_FEAT_ELEV_LIMIT;
}

// norm = 1 / sqrt(lattice(ones) + 1e-20) for images [0,B); va/vb: scratch of >= (number of lattice points) floats.
int crf_lattice_norm(const CrfLattice& L, const PostDesc* d_imgs, int B, int max_pixels, size_t ent_total, float* va, float* vb,
                     float* norm_out, hipStream_t s) {
    const int D = L.D1 - 1;
    const int nb = 1024;
    hipLaunchKernelGGL(crf_splat1_kernel, dim3(nb, B), dim3(256), 0, s, L, d_imgs, va);
    float* src = va;
    float* dst = vb;
    for (int j = 0; j <= D; j++) {
        hipLaunchKernelGGL(crf_blur1_kernel, dim3(nb, B), dim3(256), 0, s, L, d_imgs, src, dst, j);
        float* t = src;
        src = dst;
        dst = t;
    }
    const int nbp = (max_pixels + 255) / 256 < 512 ? (max_pixels + 255) / 256 : 512;
    hipLaunchKernelGGL(crf_norm_kernel, dim3(nbp, B), dim3(256), 0, s, L, d_imgs, src, norm_out, crf_alpha(D));
    hipLaunchKernelGGL(entry_norm_kernel, dim3(2048), dim3(256), 0, s, L.ent, ent_total, norm_out);
    return ok();
}

}  // namespace pnp
