// Internal to csrc/, included only by crf_lattice.hip and, through crf_tile.h, by crf_meanfield.hip and crf_grad.hip: the device
// helpers and constants the DenseCRF kernels of those units share, and the host-side helpers their launchers share.  The pieces
// of the tiled update / backward kernels (tile geometry, item walk, slice records, slice, label, store loop): crf_tile.h.
// The algorithm: crf_lattice.hip.
#pragma once
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "../../include/pnp_math.h"

namespace pnp {

// Streaming accesses of the mean-field kernels (data with no reuse inside a launch: contributor records, the value rows a splat
// writes, the unary rows an update reads and the Q rows it writes) are marked non-temporal, so that they do not displace the
// rows that ARE reused (a pixel's Q row is gathered by its 3 + 6 lattice points) from L2.  Round 5, same-box A/B
// (plain against non-temporal accesses, two alternations): mean-field per step 30.9 / 30.6 -> 30.3 / 30.6 ms on the headline batch (neutral),
// 74.1 / 75.0 -> 72.5 / 72.9 ms at K = 59, 72.3 / 72.3 -> 67.3 / 71.1 ms at 3.6 lattice points per pixel, 252 / 257 -> 253 / 253 ms
// at ADE20K size: small, never negative; the stores of the two-axis lattice blur on top of that: 30.6 / 30.8 -> 30.3 / 29.6 ms
// (headline), 74.8 / 74.2 -> 73.1 / 73.1 (K = 59), 71.6 / 71.5 -> 69.7 / 66.6 (3.6 points per pixel).  Loads / stores are otherwise
// identical: results unchanged.
template <typename T> __device__ __forceinline__ T ld_stream(const T* p) { return __builtin_nontemporal_load(p); }
template <typename T> __device__ __forceinline__ void st_stream(T* p, const T& v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ CrfEntry ld_entry(const CrfEntry* p) {
    return __builtin_bit_cast(CrfEntry, ld_stream(reinterpret_cast<const chunk16*>(p)));
}

// One element of a lattice axis blur, densecrf's `old + 0.5 * (n1 + n2)` (double literal): (n1 + n2) is a float sum; the
// product by 0.5 is exact; and the double sum old + 0.5 t, rounded to float, equals the single rounding of the exact sum
// (it is exact in double whenever the exponents are within 28, and beyond that the small term is below a quarter ulp of the
// float result on either path) -- i.e. one float fma.  Two VALU instructions per element instead of two conversions, an
// fp64 multiply, an fp64 add and a conversion back; bit-identical to the oracle's double form (tests: GPU == oracle).
__device__ __forceinline__ float crf_axis(float old, float n1, float n2) { return __fmaf_rn(0.5f, __fadd_rn(n1, n2), old); }

// Work distribution of the iteration kernels: workgroups with the same blockIdx % 8 share an XCD
// (round-robin dispatch; a speed assumption only), so each XCD is given whole images (b = xcd,
// xcd + 8, ...) and sweeps them one after another: the ~10 MB value rows of the image an XCD is
// working on are re-read (neighbour / contributor gathers) out of L2 / Infinity Cache instead of HBM.
// Inside an image LPP lanes share one lattice point (one 16-byte channel chunk each); LPP = 8, 16 or 32 is the
// smallest that covers the widest row of the batch, so the contributor list of a point is walked once
// (with LPP = 8 a 36-float row walked it twice: +43 % on the whole mean-field pass).
//
// Image schedule of an XCD: whole images img0 + xcd, + 8, ... while a full round of 8 remains; the last nimg % 8 images
// are cut into 8 equal slices, one per XCD (with 35 images three XCDs would otherwise sweep a fifth image while five
// idle: 12.5 % of every iteration kernel).
__device__ __forceinline__ bool xcd_work(int i, int xcd, int img0, int nimg, int& b, int& part, int& parts) {
    const int full = nimg >> 3;
    if (i < full) {
        b = img0 + i * 8 + xcd;
        part = 0;
        parts = 1;
        return true;
    }
    if (i - full < (nimg & 7)) {
        b = img0 + full * 8 + (i - full);
        part = xcd;
        parts = 8;
        return true;
    }
    return false;
}

// pixels of the largest tile of the update kernels (crf_update_kernel, crf_meanfield.hip: a TW x TH block, crf_tile_w wide)
constexpr int CRF_TP = 256;
// channels per group from which the update's softmax runs wave-parallel (see there).  Measured (tools/cfg_kstats.sh): K = 150 (32-pixel
// tiles, 64 rows: the thread-per-row form keeps ONE wave busy) 1350 -> 1169 us per launch; K = 81 / 59 (64 / 128 rows) 1654 -> 2514 /
// 1947 -> 3029 us -- a row's dependent chain (LDS read, six shuffles, exponential, store) is too long where rows are many and short
constexpr int CRF_WAVE_SOFTMAX_K = 128;
__host__ __device__ inline int crf_tile_w(int tp) { return tp >= 128 ? 16 : tp >= 32 ? 8 : 4; }
// labels per block of the compatibility products (crf_update_compat_kernel, crf_meanfield.hip): the transposed matrices' row
// stride is a multiple of it
constexpr int CRF_CL = 8;

// ------------------------------------------------------------------------------------------ host
static inline int ok() { return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP; }

static float crf_alpha(int D) { return 1.0f / (1 + powf(2, (float)-D)); }

// f(std::integral_constant<int, D>()) for the run-time d = D in LO .. HI: a kernel's template argument from a lattice's
// dimension.  Beyond the range: PNP_ERR_ARG
template <int LO, int HI, typename F>
static int crf_dispatch(int d, F&& f) {
    if constexpr (LO > HI) return PNP_ERR_ARG;
    else return d == LO ? f(std::integral_constant<int, LO>()) : crf_dispatch<LO + 1, HI>(d, f);
}

// Grid of the XCD-affine iteration kernels: 8 XCD groups x the workgroups that are RESIDENT per XCD for this kernel
// (occupancy query x CUs per XCD).  Each workgroup walks its share of every image of its XCD, so a grid larger than what is
// resident runs as a second wave of workgroups after the first has swept all its images: unbalanced, and the second wave
// re-fetches from HBM every Q / value row the first one had in L2.
template <typename F>
static int resident_grid(F kernel, int threads, size_t smem) {
    int cus = device_cu_count(), occ = 0;
    if (cus <= 0) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, smem) != hipSuccess || occ < 1) occ = 1;
    const int per_xcd = (cus / 8 > 0 ? cus / 8 : 1) * occ;
    return 8 * (per_xcd < 256 ? per_xcd : 256);
}

// The one table of crf_launch_tiled's grids, by (kernel, device, LDS bytes): the occupancy depends on the tile's LDS bytes, a
// handful of sizes per process.  Engines of different host threads / devices share it.  store = 0: look up (0: not there)
inline int crf_tiled_grid(const void* kernel, int dev, size_t smem, int store) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, size_t>, int> grids;
    std::lock_guard<std::mutex> lk(mu);
    int& nb = grids[std::make_tuple(kernel, dev, smem)];
    if (store) nb = store;
    return nb;
}

// Launch of a kernel that keeps a tile in `smem` bytes of dynamic LDS: the limit raised where a tile passes 64 KB (the CU has
// 160), 256 threads, the resident grid for these LDS bytes
template <typename... P, typename... A>
static int crf_launch_tiled(void (*kernel)(P...), size_t smem, hipStream_t s, const A&... args) {
    if (smem > 160 * 1024) return PNP_ERR_ARG;
    const void* const key = reinterpret_cast<const void*>(kernel);
    if (smem > 64 * 1024) {
        if (hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return PNP_ERR_HIP;
    }
    const int dev = current_device();
    int nb = crf_tiled_grid(key, dev, smem, 0);
    if (!nb) nb = crf_tiled_grid(key, dev, smem, resident_grid(kernel, 256, smem));
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), smem, s, args...);
    return ok();
}

// LDS rows per pixel and pixels per tile of crf_term_update_kernel / crf_term_backward_kernel (see there):
// crf_compat_tile_pixels' rule on their own rows
static int crf_term_tile_pixels(int max_kp, int D1, int rows, size_t* smem) {
    const size_t per_pixel = ((size_t)rows * (max_kp + 1) + 2 * D1 + 1) * sizeof(float);
    int tp = 256;
    while (tp > 64 && tp * per_pixel > 64 * 1024) tp >>= 1;
    if (tp * per_pixel > 158 * 1024) tp = 32;
    *smem = tp * per_pixel;
    return tp;
}

}  // namespace pnp
