// Baseline JPEG encode on gfx950: the inverse of jpeg.hip, for images that already sit in HBM (overlays of label maps).  The
// files equal Pillow's `Image.save(buf, "JPEG", quality=q)` byte for byte: libjpeg's defaults (YCbCr 4:2:0, the "islow" integer
// DCT, the T.81 Annex K Huffman tables, no restart markers), restated from the published algorithm (tests/_vis_refs.py, pinned
// against Pillow).  The host writes the markers (pnp_ovss/jpeg.py); the device produces the entropy-coded scan of every image
// of a batch:
//   jpeg_enc_transform_kernel  one workgroup per strip of 4 MCUs (64 x 16 pixels).  Colour conversion (jccolor.c fixed point),
//                              edge replication, h2v2 chroma downsampling with the alternating 1, 2 bias (jcsample.c), staged
//                              in LDS as six 8 x 8 blocks per MCU; jfdctint.c rows then columns, one thread per row / column;
//                              quantisation (jcdctmgr.c); the blocks leave in zig-zag order, in scan order (Y00 Y01 Y10 Y11 Cb
//                              Cr per MCU).  Luma blocks of the MCU grid that lie wholly outside the image are libjpeg's
//                              dummy blocks: AC 0, DC of the block in front of them in the MCU, so their DC difference is 0.
//   jpeg_enc_bits_kernel       one thread per block: its DC difference against the previous block of the same component (a
//                              direct index in scan order) and the bit length of its Huffman codes.
//   (device_scan_i32)          exclusive prefix sum of the bit lengths over the whole batch: a block's bit offset inside its
//                              image is the difference to the image's first block.
//   jpeg_enc_pack_kernel       one thread per block emits its codes at its bit offset into the image's zeroed big-endian
//                              words: plain stores for the words it owns, atomicOr for its first and last word, which it may
//                              share with a neighbour.  The image's last block appends the 1-bits that fill the final byte.
//   jpeg_enc_ffcount_kernel    one thread per 64-byte chunk of the packed stream counts its 0xFF bytes,
//   (device_scan_i32)          the counts are prefix-summed,
//   jpeg_enc_stuff_kernel      and every chunk is copied to its place in the output with a 0x00 behind each 0xFF.
// An image whose scan does not fit its declared capacity (known once the 0xFF bytes are counted) sets *d_err, gets out_len -1
// and not one byte written; the other images of the batch are unaffected.  Integer VALU and LDS only; no host read-back.
#include <vector>

#include "common.h"
#include "kernels.h"
#include "../../include/pnp_hip.h"

namespace pnp {

static __constant__ int kEncZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kEncStripMcus = 4;       // MCUs per workgroup of the transform
constexpr int kEncChunk = 64;          // bytes of packed stream per thread of the stuffing passes
constexpr int kEncMaxBlockBits = 1664; // >= 20 (DC: 9 + 11) + 63 * 26 (AC: 16 + 10) bits of one block

struct EncImage {          // device-side descriptor: the caller's pnp_jpeg_enc_image plus the derived geometry
    int64_t rgb_off, out_off, word_off;
    int32_t H, W, cap, mcux, mcuy;
    int32_t mcu0, strip0, chunk0;      // first MCU / transform strip / stuffing chunk of the image in the batch-wide numbering
};
struct EncTables {         // [DC luma, DC chroma, AC luma, AC chroma] canonical codes by symbol
    uint16_t code[4][256];
    uint8_t len[4][256];
};
struct EncQuant {
    uint16_t q[2][64];     // luma, chroma; natural order
};

// index of the image that owns batch-wide item `idx`: the last one whose first item (member F) is <= idx
template <int32_t EncImage::*F> __device__ __forceinline__ int enc_find_image(const EncImage* __restrict__ imgs, int B, int idx) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].*F <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one 1-D pass over d[0..7] (CONST_BITS 13, PASS1_BITS 2): FIRST = the row pass (results scaled up by 4)
template <bool FIRST> __device__ __forceinline__ void enc_fdct8(int* d) {
    constexpr int CB = 13, P1 = 2, N = FIRST ? CB - P1 : CB + P1;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * (1 << P1);
        d[4] = (t10 - t11) * (1 << P1);
    } else {
        d[0] = enc_descale(t10 + t11, P1);
        d[4] = enc_descale(t10 - t11, P1);
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = enc_descale(z1 + t13 * 6270, N);
    d[6] = enc_descale(z1 + t12 * (-15137), N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    d[7] = enc_descale(u4 + z1 + z3, N);
    d[5] = enc_descale(u5 + z2 + z4, N);
    d[3] = enc_descale(u6 + z2 + z3, N);
    d[1] = enc_descale(u7 + z1 + z4, N);
}

// ------------------------------------------------------------------------------------------ colour, downsample, FDCT, quantise
__global__ __launch_bounds__(256) void jpeg_enc_transform_kernel(const uint8_t* __restrict__ rgb, const EncImage* __restrict__ imgs, int B,
                                                                 const EncQuant qt, int16_t* __restrict__ coef) {
    __shared__ int samp[kEncStripMcus][6][64];
    const int tid = threadIdx.x;
    const int ii = enc_find_image<&EncImage::strip0>(imgs, B, (int)blockIdx.x);
    const EncImage im = imgs[ii];
    const int spr = (im.mcux + kEncStripMcus - 1) / kEncStripMcus;     // strips per MCU row
    const int s = (int)blockIdx.x - im.strip0;
    const int my = s / spr, mx0 = (s % spr) * kEncStripMcus;
    const int nm = min(kEncStripMcus, im.mcux - mx0);
    const uint8_t* src = rgb + im.rgb_off;
    const int H = im.H, W = im.W;
    // luma: 64 x 16 pixels of the strip, columns and rows beyond the image repeat the last one
    for (int p = tid; p < 64 * 16; p += 256) {
        const int px = p & 63, py = p >> 6, m = px >> 4;
        if (m >= nm) continue;
        const int x = min(mx0 * 16 + px, W - 1), y = min(my * 16 + py, H - 1);
        const uint8_t* q = src + ((size_t)y * W + x) * 3;
        const int r = q[0], g = q[1], b = q[2];
        samp[m][((py >> 3) << 1) | ((px >> 3) & 1)][(py & 7) * 8 + (px & 7)] = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    }
    // chroma: one thread per downsampled sample.  Columns: the full-resolution row is extended by its last pixel.  Rows: an odd
    // height repeats the last full-resolution row to finish the pair; further rows repeat the last DOWNSAMPLED row.
    {
        const int m = tid >> 6, cy = (tid >> 3) & 7, cxl = tid & 7;
        if (m < nm) {
            const int cx = (mx0 + m) * 8 + cxl;
            const int cyg = min(my * 8 + cy, (H + 1) / 2 - 1);
            const int y0 = 2 * cyg, y1 = min(2 * cyg + 1, H - 1);
            const int x0 = min(2 * cx, W - 1), x1 = min(2 * cx + 1, W - 1);
            int sb = 0, sr = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint8_t* q = src + ((size_t)((k & 2) ? y1 : y0) * W + ((k & 1) ? x1 : x0)) * 3;
                const int r = q[0], g = q[1], b = q[2];
                sb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
                sr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            }
            const int bias = (cxl & 1) ? 2 : 1;
            samp[m][4][cy * 8 + cxl] = (sb + bias) >> 2;
            samp[m][5][cy * 8 + cxl] = (sr + bias) >> 2;
        }
    }
    __syncthreads();
    const int blk = tid >> 3, line = tid & 7;          // 24 blocks x 8 rows / columns on the first 192 threads
    const int bm = blk / 6, bk = blk % 6;
    const bool active = tid < kEncStripMcus * 6 * 8 && bm < nm;
    // real luma blocks reach into the image; the others of the MCU grid are dummies
    const int bxr = (W + 7) >> 3, byr = (H + 7) >> 3;
    const int lx = (mx0 + bm) * 2 + (bk & 1), ly = my * 2 + (bk >> 1);
    const bool col_dummy = bk < 4 && ((mx0 + bm) * 2 + 1) >= bxr, row_dummy = bk < 4 && (my * 2 + 1) >= byr;
    const bool dummy = bk < 4 && (lx >= bxr || ly >= byr);
    int d[8];
    if (active && !dummy) {
        int* row = &samp[bm][bk][line * 8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = row[i] - 128;
        enc_fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; i++) row[i] = d[i];
    }
    __syncthreads();
    if (active && !dummy) {
        int* col = &samp[bm][bk][line];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = col[i * 8];
        enc_fdct8<false>(d);
        const uint16_t* q = qt.q[bk < 4 ? 0 : 1];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int q8 = (int)q[i * 8 + line] << 3;       // the DCT output carries a factor of 8
            const int a = (abs(d[i]) + (q8 >> 1)) / q8;
            col[i * 8] = d[i] < 0 ? -a : a;
        }
    }
    __syncthreads();
    if (active) {
        // the dummy's DC: right-edge dummy -> the block to its left; bottom-row dummy -> block 1 of the MCU (itself block 0's
        // copy when it is a dummy too)
        int srcb = bk;
        if (dummy) srcb = bk == 1 ? 0 : bk == 2 ? (col_dummy ? 0 : 1) : (row_dummy ? (col_dummy ? 0 : 1) : 2);
        const int* sb = samp[bm][srcb];
        int16_t* dst = coef + ((size_t)(im.mcu0 + my * im.mcux + mx0 + bm) * 6 + bk) * 64 + line * 8;
        union { int16_t h[8]; chunk16 v; } o;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int z = line * 8 + i;
            o.h[i] = dummy ? (z == 0 ? (int16_t)sb[0] : (int16_t)0) : (int16_t)sb[kEncZigzag[z]];
        }
        *reinterpret_cast<chunk16*>(dst) = o.v;
    }
}

// ------------------------------------------------------------------------------------------ entropy coding of one block
// T.81 F.1.2: the DC difference by category + extra bits, then (run, size) symbols with ZRL for runs above 15 and EOB when the
// block ends in zeros.  `E::put(code, len)` receives every code word, len <= 27 bits.
template <class E> __device__ __forceinline__ void enc_ac(E& e, int v, int& run, const uint16_t* code, const uint8_t* len) {
    if (v == 0) {
        run++;
        return;
    }
    while (run > 15) {
        e.put(code[0xF0], len[0xF0]);
        run -= 16;
    }
    const int a = abs(v), n = 32 - __clz(a), sym = (run << 4) | n;
    e.put(((uint32_t)code[sym] << n) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << n) - 1)), len[sym] + n);
    run = 0;
}

template <class E> __device__ __forceinline__ void enc_block(E& e, const int16_t* __restrict__ blk, int pred, const EncTables& T, int chroma) {
    const chunk16* p = reinterpret_cast<const chunk16*>(blk);
    const uint16_t* dcode = T.code[chroma];
    const uint8_t* dlen = T.len[chroma];
    const uint16_t* acode = T.code[2 + chroma];
    const uint8_t* alen = T.len[2 + chroma];
    int run = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        union { chunk16 v; int16_t h[8]; } u;
        u.v = p[j];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int v = u.h[i];
            if (j == 0 && i == 0) {
                const int diff = v - pred;
                const int n = diff ? 32 - __clz(abs(diff)) : 0;
                e.put(((uint32_t)dcode[n] << n) | (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << n) - 1)), dlen[n] + n);
            } else {
                enc_ac(e, v, run, acode, alen);
            }
        }
    }
    if (run > 0) e.put(acode[0], alen[0]);
}

struct EncCounter {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
};
struct EncWriter {          // big-endian bit writer into zeroed 32-bit words; the first and the last word may be shared
    uint32_t* w;
    uint64_t acc = 0;
    int n;
    bool first = true;
    __device__ __forceinline__ void put(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            const uint32_t word = (uint32_t)(acc >> (n - 32));
            if (first) atomicOr(w, word);
            else *w = word;
            first = false;
            w++;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(w, (uint32_t)(acc << (32 - n)));
    }
};

__device__ __forceinline__ void enc_load_tables(EncTables& sh, const EncTables* __restrict__ g) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(g);
    uint32_t* d = reinterpret_cast<uint32_t*>(&sh);
    for (int i = threadIdx.x; i < (int)(sizeof(EncTables) / 4); i += blockDim.x) d[i] = s[i];
    __syncthreads();
}

// DC predictor of batch-wide block g (component k of MCU m): luma -> the previous luma block in scan order, chroma -> the same
// component of the previous MCU; 0 at the image's first MCU
__device__ __forceinline__ int enc_pred(const int16_t* __restrict__ coef, int g, int k, bool first_mcu) {
    if (k >= 1 && k <= 3) return coef[(size_t)(g - 1) * 64];
    if (first_mcu) return 0;
    return coef[(size_t)(g - (k == 0 ? 3 : 6)) * 64];
}

__global__ __launch_bounds__(256) void jpeg_enc_bits_kernel(const int16_t* __restrict__ coef, const EncImage* __restrict__ imgs, int B,
                                                            const EncTables* __restrict__ tabs, int nblocks, int* __restrict__ nbits) {
    __shared__ EncTables T;
    enc_load_tables(T, tabs);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nblocks) return;
    const int m = g / 6, k = g - m * 6;
    const int ii = enc_find_image<&EncImage::mcu0>(imgs, B, m);
    EncCounter c;
    enc_block(c, coef + (size_t)g * 64, enc_pred(coef, g, k, m == imgs[ii].mcu0), T, k >= 4);
    nbits[g] = c.bits;
}

// bits of image `im`'s whole scan, before the padding of its last byte
__device__ __forceinline__ int enc_total_bits(const EncImage& im, const int* __restrict__ nbits, const int* __restrict__ boff) {
    const int g0 = im.mcu0 * 6, gl = g0 + im.mcux * im.mcuy * 6 - 1;
    return boff[gl] + nbits[gl] - boff[g0];
}

__global__ __launch_bounds__(256) void jpeg_enc_pack_kernel(const int16_t* __restrict__ coef, const EncImage* __restrict__ imgs, int B,
                                                            const EncTables* __restrict__ tabs, int nblocks, const int* __restrict__ nbits,
                                                            const int* __restrict__ boff, uint32_t* __restrict__ words) {
    __shared__ EncTables T;
    enc_load_tables(T, tabs);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nblocks) return;
    const int m = g / 6, k = g - m * 6;
    const int ii = enc_find_image<&EncImage::mcu0>(imgs, B, m);
    const EncImage im = imgs[ii];
    const int total = enc_total_bits(im, nbits, boff);
    if ((total + 7) / 8 > im.cap) return;               // does not fit: nothing of this image is written
    const int off = boff[g] - boff[im.mcu0 * 6];
    EncWriter e;
    e.w = words + im.word_off + (off >> 5);
    e.n = off & 31;
    enc_block(e, coef + (size_t)g * 64, enc_pred(coef, g, k, m == im.mcu0), T, k >= 4);
    if (g == im.mcu0 * 6 + im.mcux * im.mcuy * 6 - 1) {
        const int pad = (-total) & 7;                   // the final byte is completed with 1-bits
        if (pad) e.put((1u << pad) - 1, pad);
    }
    e.finish();
}

// ------------------------------------------------------------------------------------------ 0xFF 0x00 stuffing
__device__ __forceinline__ uint32_t enc_byte(const uint32_t* __restrict__ w, int j) { return (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF; }

__global__ __launch_bounds__(256) void jpeg_enc_ffcount_kernel(const EncImage* __restrict__ imgs, int B, int nchunks, const int* __restrict__ nbits,
                                                               const int* __restrict__ boff, const uint32_t* __restrict__ words,
                                                               int* __restrict__ ffcnt) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    const int ii = enc_find_image<&EncImage::chunk0>(imgs, B, c);
    const EncImage im = imgs[ii];
    const int n = (enc_total_bits(im, nbits, boff) + 7) / 8;
    int cnt = 0;
    if (n <= im.cap) {
        const int j0 = (c - im.chunk0) * kEncChunk, j1 = min(n, j0 + kEncChunk);
        const uint32_t* w = words + im.word_off;
        for (int j = j0; j < j1; j++) cnt += enc_byte(w, j) == 0xFF;
    }
    ffcnt[c] = cnt;
}

__global__ __launch_bounds__(256) void jpeg_enc_stuff_kernel(const EncImage* __restrict__ imgs, int B, int nchunks, const int* __restrict__ nbits,
                                                             const int* __restrict__ boff, const uint32_t* __restrict__ words,
                                                             const int* __restrict__ ffcnt, const int* __restrict__ ffoff,
                                                             uint8_t* __restrict__ out, int* __restrict__ out_len, int* __restrict__ err) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    const int ii = enc_find_image<&EncImage::chunk0>(imgs, B, c);
    const EncImage im = imgs[ii];
    const int n = (enc_total_bits(im, nbits, boff) + 7) / 8;
    const int cl = im.chunk0 + (im.cap + kEncChunk - 1) / kEncChunk - 1;       // the image's last chunk
    const int total = n + (ffoff[cl] + ffcnt[cl] - ffoff[im.chunk0]);
    const bool fits = n <= im.cap && total <= im.cap;
    if (c == im.chunk0) {
        out_len[ii] = fits ? total : -1;
        if (!fits) *err = 1;
    }
    if (!fits) return;
    const int j0 = (c - im.chunk0) * kEncChunk, j1 = min(n, j0 + kEncChunk);
    const uint32_t* w = words + im.word_off;
    uint8_t* dst = out + im.out_off + j0 + (ffoff[c] - ffoff[im.chunk0]);
    for (int j = j0; j < j1; j++) {
        const uint32_t b = enc_byte(w, j);
        *dst++ = (uint8_t)b;
        if (b == 0xFF) *dst++ = 0;
    }
}

// T.81 Annex K.3 tables (codes per length 1..16, symbols), and Annex C: canonical codes in symbol order
static const uint8_t kDcLumaCounts[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kDcChromaCounts[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcLumaCounts[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static const uint8_t kAcChromaCounts[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

static void enc_fill_table(EncTables& T, int t, const uint8_t* counts, const uint8_t* vals) {
    int code = 0, k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < counts[len - 1]; i++, k++, code++) {
            T.code[t][vals[k]] = (uint16_t)code;
            T.len[t][vals[k]] = (uint8_t)len;
        }
        code <<= 1;
    }
}

static inline size_t enc_align(size_t v) { return (v + 255) & ~(size_t)255; }

int jpeg_encode(const uint8_t* d_rgb, const pnp_jpeg_enc_image* h_imgs, int B, const uint16_t* h_quant, uint8_t* d_out, int* d_out_len,
                int* d_err, void* d_ws, int64_t ws_bytes, int64_t* ws_need, hipStream_t s) {
    if (!h_imgs || B < 1 || !h_quant) return PNP_ERR_ARG;
    std::vector<EncImage> im((size_t)B);
    int64_t mcus = 0, strips = 0, chunks = 0, words = 0;
    for (int i = 0; i < B; i++) {
        const pnp_jpeg_enc_image& h = h_imgs[i];
        if (h.H < 1 || h.W < 1 || h.H > 65535 || h.W > 65535 || h.out_cap < 1 || h.rgb_off < 0 || h.out_off < 0) return PNP_ERR_ARG;
        EncImage& e = im[(size_t)i];
        e.rgb_off = h.rgb_off;
        e.out_off = h.out_off;
        e.word_off = words;
        e.H = h.H;
        e.W = h.W;
        e.cap = h.out_cap;
        e.mcux = (h.W + 15) / 16;
        e.mcuy = (h.H + 15) / 16;
        e.mcu0 = (int32_t)mcus;
        e.strip0 = (int32_t)strips;
        e.chunk0 = (int32_t)chunks;
        mcus += (int64_t)e.mcux * e.mcuy;
        strips += (int64_t)e.mcuy * ((e.mcux + kEncStripMcus - 1) / kEncStripMcus);
        chunks += (h.out_cap + kEncChunk - 1) / kEncChunk;
        words += (h.out_cap + 3) / 4 + 2;                 // the packed stream never exceeds the capacity (checked before a bit is written)
        // batch-wide bit offsets and item numbers are int32
        if (mcus * 6 * kEncMaxBlockBits >= ((int64_t)1 << 31) || chunks >= ((int64_t)1 << 30) || words >= ((int64_t)1 << 31)) return PNP_ERR_ARG;
    }
    for (int k = 0; k < 128; k++)
        if (h_quant[k] < 1 || h_quant[k] > 255) return PNP_ERR_ARG;
    const size_t nblocks = (size_t)mcus * 6;
    const size_t scan_n = nblocks > (size_t)chunks ? nblocks : (size_t)chunks;
    size_t o = 0;
    const size_t o_img = o;    o += enc_align(sizeof(EncImage) * (size_t)B);
    const size_t o_tab = o;    o += enc_align(sizeof(EncTables));
    const size_t o_coef = o;   o += enc_align(nblocks * 64 * sizeof(int16_t));
    const size_t o_nbits = o;  o += enc_align(nblocks * sizeof(int));
    const size_t o_boff = o;   o += enc_align(nblocks * sizeof(int));
    const size_t o_words = o;  o += enc_align((size_t)words * sizeof(uint32_t));
    const size_t o_ffcnt = o;  o += enc_align((size_t)chunks * sizeof(int));
    const size_t o_ffoff = o;  o += enc_align((size_t)chunks * sizeof(int));
    const size_t o_tmp = o;
    const size_t tmp_bytes = sort_temp_bytes(scan_n);
    o += enc_align(tmp_bytes);
    if (ws_need) *ws_need = (int64_t)o;
    if (!d_ws) return ws_need ? PNP_OK : PNP_ERR_ARG;
    if (!d_rgb || !d_out || !d_out_len || !d_err || ws_bytes < (int64_t)o) return PNP_ERR_ARG;

    static const EncTables tables = [] {
        EncTables T{};
        enc_fill_table(T, 0, kDcLumaCounts, kDcVals);
        enc_fill_table(T, 1, kDcChromaCounts, kDcVals);
        enc_fill_table(T, 2, kAcLumaCounts, kAcLumaVals);
        enc_fill_table(T, 3, kAcChromaCounts, kAcChromaVals);
        return T;
    }();
    EncQuant qt;
    for (int k = 0; k < 128; k++) qt.q[k / 64][k % 64] = h_quant[k];
    uint8_t* ws = reinterpret_cast<uint8_t*>(d_ws);
    EncImage* d_img = reinterpret_cast<EncImage*>(ws + o_img);
    EncTables* d_tab = reinterpret_cast<EncTables*>(ws + o_tab);
    int16_t* d_coef = reinterpret_cast<int16_t*>(ws + o_coef);
    int* d_nbits = reinterpret_cast<int*>(ws + o_nbits);
    int* d_boff = reinterpret_cast<int*>(ws + o_boff);
    uint32_t* d_words = reinterpret_cast<uint32_t*>(ws + o_words);
    int* d_ffcnt = reinterpret_cast<int*>(ws + o_ffcnt);
    int* d_ffoff = reinterpret_cast<int*>(ws + o_ffoff);
    if (hipMemcpyAsync(d_img, im.data(), sizeof(EncImage) * (size_t)B, hipMemcpyHostToDevice, s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemcpyAsync(d_tab, &tables, sizeof(EncTables), hipMemcpyHostToDevice, s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemsetAsync(d_words, 0, (size_t)words * sizeof(uint32_t), s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemsetAsync(d_err, 0, sizeof(int), s) != hipSuccess) return PNP_ERR_HIP;
    const unsigned gb = (unsigned)((nblocks + 255) / 256), gc = (unsigned)((chunks + 255) / 256);
    hipLaunchKernelGGL(jpeg_enc_transform_kernel, dim3((unsigned)strips), dim3(256), 0, s, d_rgb, (const EncImage*)d_img, B, qt, d_coef);
    hipLaunchKernelGGL(jpeg_enc_bits_kernel, dim3(gb), dim3(256), 0, s, (const int16_t*)d_coef, (const EncImage*)d_img, B,
                       (const EncTables*)d_tab, (int)nblocks, d_nbits);
    int r = device_scan_i32(d_nbits, d_boff, nblocks, false, ws + o_tmp, tmp_bytes, s);
    if (r != PNP_OK) return r;
    hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3(gb), dim3(256), 0, s, (const int16_t*)d_coef, (const EncImage*)d_img, B,
                       (const EncTables*)d_tab, (int)nblocks, (const int*)d_nbits, (const int*)d_boff, d_words);
    hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, dim3(gc), dim3(256), 0, s, (const EncImage*)d_img, B, (int)chunks, (const int*)d_nbits,
                       (const int*)d_boff, (const uint32_t*)d_words, d_ffcnt);
    r = device_scan_i32(d_ffcnt, d_ffoff, (size_t)chunks, false, ws + o_tmp, tmp_bytes, s);
    if (r != PNP_OK) return r;
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(gc), dim3(256), 0, s, (const EncImage*)d_img, B, (int)chunks, (const int*)d_nbits,
                       (const int*)d_boff, (const uint32_t*)d_words, (const int*)d_ffcnt, (const int*)d_ffoff, d_out, d_out_len, d_err);
    return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP;
}

}  // namespace pnp

extern "C" int pnp_jpeg_encode(const uint8_t* d_rgb, const pnp_jpeg_enc_image* h_images, int32_t n_images, const uint16_t* h_quant,
                               uint8_t* d_out, int32_t* d_out_len, int32_t* d_err, void* d_ws, int64_t ws_bytes, int64_t* ws_need,
                               void* stream) {
    return pnp::jpeg_encode(d_rgb, h_images, n_images, h_quant, d_out, d_out_len, d_err, d_ws, ws_bytes, ws_need, (hipStream_t)stream);
}
