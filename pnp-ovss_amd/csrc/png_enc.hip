// Indexed-PNG encode of label maps on gfx950: the zlib stream of an 8-bit PNG's IDAT chunk for every uint8 label map of a batch
// that already sits in HBM (what pnp_remap_hist leaves).  The host writes the chunk framing and its CRC-32 around the stream
// (pnp_ovss/png.py).  The byte format is fixed (tests/_png_refs.py restates it from RFC 1950 / 1951 / the PNG specification):
//   zlib header 78 01; ONE deflate block, BFINAL = 1, BTYPE = 01 (the fixed Huffman code); end-of-block; zero bits up to a whole
//   byte; the Adler-32 of the filtered stream, big-endian.
//   Filtered stream, row y: R = the W label bytes, U[x] = (R_y[x] - R_{y-1}[x]) mod 256 with R_{-1} = 0; c0 / c2 = the number of
//   x in 1..W-1 where R / U differs from its left neighbour; the row is (2, U) when c2 < c0 and (0, R) otherwise.
//   Tokens: the W + 1 bytes of a row, filter byte included, are cut into maximal runs of equal bytes (a run never crosses a
//   row).  A run of byte b and length r is: literal b; floor((r - 1) / 258) matches of length 258 at distance 1; then with
//   t = (r - 1) mod 258 one match of length t at distance 1 when t >= 3, t literals b otherwise.
// Stages, all over the whole batch (element = one byte of a filtered stream, N of them; run numbers are batch-wide):
//   png_filter_kernel   one workgroup per row: c0 and c2, the filter choice, the filtered row, a flag on every run head, and the
//                       row's Adler-32 share.  With n = H (W + 1) bytes d_i in an image, A = 1 + sum d_i and
//                       B = n + sum (n - i) d_i; for byte j of row y, n - i = (H - 1 - y)(W + 1) + (W + 1 - j), so a row gives
//                       S = sum d and (H - 1 - y)(W + 1) S + sum (W + 1 - j) d_j, in 64-bit integers, stored mod 65521.
//   (device_scan_i32)   exclusive prefix sum of the head flags: the number of every run.
//   png_runs_kernel     every head writes its element index at its run number; the last element also writes the run count R
//                       and the end sentinel, so a run's length is the distance to the next head.
//   png_bits_kernel     one thread per run: the bit length of its code words (0 behind run R).
//   (device_scan_i32)   exclusive prefix sum of the bit lengths: a run's bit offset inside its image is 19 (the zlib header and
//                       the three block-header bits) + the difference to the image's first run.
//   png_pack_kernel     one thread per run writes its code words at its bit offset into the image's zeroed little-endian words
//                       (deflate's bit order is LSB first, so bit k of the stream is bit k & 31 of word k >> 5): plain stores
//                       for the words it owns, atomicOr for its first and last word, which it may share with a neighbour.
//                       Huffman codes are bit-reversed once, in the tables.  A run costs at most 254 matches + 3 code words.
//   png_finish_kernel   one workgroup per image: sums the rows' Adler shares, ORs the header bytes, the block header and the
//                       four Adler bytes into the words (end-of-block and the padding are zero bits: already there), and
//                       writes the length, or -1 and *d_err = 1 when the stream exceeds the image's capacity.
//   png_copy_kernel     one thread per word: the bytes of every image that fits go to d_out + out_off (any alignment).
// The words are sized by the worst case of the format, not by the caller's capacity, so an image that does not fit is packed
// like any other and simply not copied: not one byte of it reaches d_out and the other images are unaffected.
// Integer VALU and LDS only; no floating point, no host read-back.
#include <vector>

#include "common.h"
#include "kernels.h"
#include "../../include/pnp_hip.h"

namespace pnp {

constexpr uint32_t kAdlerMod = 65521;
constexpr int64_t kPngMaxElems = ((int64_t)1 << 31) / 9;       // per call: bit offsets go through the int32 scan, <= 9 bits per byte

struct PngImage {          // device-side descriptor: the caller's pnp_png_image plus the derived numbering
    int64_t lab_off, out_off;
    int32_t H, W, cap;
    int32_t row0, elem0, word0;        // first row / filtered byte / packed word of the image in the batch-wide numbering
};
struct PngTables {
    uint32_t match[256];   // length L = 3 .. 258 at [L - 3]: (bits << 24) | reversed length code | extra bits above it; the
                           // five zero bits of distance code 0 are counted in `bits`
    uint16_t lit[256];     // literal b: its 8-bit (b < 144) or 9-bit code, reversed
};

template <int32_t PngImage::*F> __device__ __forceinline__ int png_find_image(const PngImage* __restrict__ imgs, int B, int idx) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].*F <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// sums of a and b over the 256 threads of the workgroup, returned to every thread
__device__ __forceinline__ void png_block_sum2(unsigned long long& a, unsigned long long& b, unsigned long long (*red)[4]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    __syncthreads();                                    // (the previous use of `red` is over)
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}

// ------------------------------------------------------------------------------------------ filter choice, run heads, Adler shares
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t* __restrict__ labels, const PngImage* __restrict__ imgs, int B,
                                                         uint8_t* __restrict__ filt, int* __restrict__ head, uint32_t* __restrict__ row_a,
                                                         uint32_t* __restrict__ row_b) {
    __shared__ unsigned long long red[2][4];
    const int tid = threadIdx.x, row = (int)blockIdx.x;
    const PngImage im = imgs[png_find_image<&PngImage::row0>(imgs, B, row)];
    const int y = row - im.row0, W = im.W, L = W + 1;
    const uint8_t* cur = labels + im.lab_off + (size_t)y * W;
    const uint8_t* prev = cur - W;                      // read only when y > 0
    unsigned long long c0 = 0, c2 = 0;
    for (int x = 1 + tid; x < W; x += 256) {
        const int r1 = cur[x], r0 = cur[x - 1];
        const int p1 = y ? prev[x] : 0, p0 = y ? prev[x - 1] : 0;
        c0 += r1 != r0;
        c2 += ((r1 - p1) & 255) != ((r0 - p0) & 255);
    }
    png_block_sum2(c0, c2, red);
    const bool up = c2 < c0;
    const int fb = up ? 2 : 0;
    const int e0 = im.elem0 + y * L;
    unsigned long long S = 0, T = 0;
    for (int j = tid; j < L; j += 256) {
        int v = fb, before = -1;                        // the filter byte heads the row's first run
        if (j > 0) {
            v = up && y ? (cur[j - 1] - prev[j - 1]) & 255 : cur[j - 1];
            before = j == 1 ? fb : (up && y ? (cur[j - 2] - prev[j - 2]) & 255 : cur[j - 2]);
        }
        filt[e0 + j] = (uint8_t)v;
        head[e0 + j] = v != before;
        S += (unsigned)v;
        T += (unsigned long long)(L - j) * (unsigned)v;
    }
    png_block_sum2(S, T, red);
    if (tid == 0) {
        const unsigned long long s = S % kAdlerMod, below = (unsigned long long)(im.H - 1 - y) * L % kAdlerMod;
        row_a[row] = (uint32_t)s;
        row_b[row] = (uint32_t)((below * s + T) % kAdlerMod);
    }
}

// ------------------------------------------------------------------------------------------ runs
__global__ __launch_bounds__(256) void png_runs_kernel(const int* __restrict__ head, const int* __restrict__ ridx, int N, int* __restrict__ runpos,
                                                       int* __restrict__ nruns) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const int h = head[e], k = ridx[e];
    if (h) runpos[k] = e;
    if (e == N - 1) {
        runpos[k + h] = N;
        *nruns = k + h;
    }
}

// The code words of a run of byte b, length r.  `E::put(code, len)` receives every code word, LSB first, len <= 18 bits.
template <class E> __device__ __forceinline__ void png_run(E& e, const PngTables* __restrict__ T, int b, int r) {
    const uint32_t lit = T->lit[b];
    const int ll = b < 144 ? 8 : 9;
    e.put(lit, ll);
    int rem = r - 1;
    const uint32_t m258 = T->match[255];
    for (; rem >= 258; rem -= 258) e.put(m258 & 0xFFFFFF, (int)(m258 >> 24));
    if (rem >= 3) {
        const uint32_t m = T->match[rem - 3];
        e.put(m & 0xFFFFFF, (int)(m >> 24));
    } else {
        for (int i = 0; i < rem; i++) e.put(lit, ll);
    }
}

struct PngCounter {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
};
struct PngWriter {          // LSB-first bit writer into zeroed little-endian 32-bit words; the first and the last word may be shared
    uint32_t* w;
    uint64_t acc = 0;
    int n;
    bool first = true;
    __device__ __forceinline__ void put(uint32_t code, int len) {
        acc |= (uint64_t)code << n;
        n += len;
        if (n >= 32) {
            if (first) atomicOr(w, (uint32_t)acc);
            else *w = (uint32_t)acc;
            first = false;
            w++;
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0 && (uint32_t)acc) atomicOr(w, (uint32_t)acc);
    }
};

__global__ __launch_bounds__(256) void png_bits_kernel(const uint8_t* __restrict__ filt, const int* __restrict__ runpos, const int* __restrict__ nruns,
                                                       const PngTables* __restrict__ tabs, int N, int* __restrict__ nbits) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > N) return;
    int bits = 0;
    if (k < *nruns) {
        const int start = runpos[k];
        PngCounter c;
        png_run(c, tabs, filt[start], runpos[k + 1] - start);
        bits = c.bits;
    }
    nbits[k] = bits;
}

__global__ __launch_bounds__(256) void png_pack_kernel(const uint8_t* __restrict__ filt, const int* __restrict__ runpos, const int* __restrict__ nruns,
                                                       const int* __restrict__ ridx, const int* __restrict__ boff, const PngImage* __restrict__ imgs,
                                                       int B, const PngTables* __restrict__ tabs, uint32_t* __restrict__ words) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= *nruns) return;
    const int start = runpos[k];
    const PngImage im = imgs[png_find_image<&PngImage::elem0>(imgs, B, start)];
    const int off = 19 + boff[k] - boff[ridx[im.elem0]];
    PngWriter e;
    e.w = words + im.word0 + (off >> 5);
    e.n = off & 31;
    png_run(e, tabs, filt[start], runpos[k + 1] - start);
    e.finish();
}

// ------------------------------------------------------------------------------------------ header, Adler-32, length
__global__ __launch_bounds__(256) void png_finish_kernel(const PngImage* __restrict__ imgs, int B, const int* __restrict__ nruns,
                                                         const int* __restrict__ ridx, const int* __restrict__ boff,
                                                         const uint32_t* __restrict__ row_a, const uint32_t* __restrict__ row_b,
                                                         uint32_t* __restrict__ words, int* __restrict__ out_len, int* __restrict__ err) {
    __shared__ unsigned long long red[2][4];
    const int i = (int)blockIdx.x;
    const PngImage im = imgs[i];
    unsigned long long sa = 0, sb = 0;                  // <= 65535 rows of values below 65521 each
    for (int y = threadIdx.x; y < im.H; y += 256) {
        sa += row_a[im.row0 + y];
        sb += row_b[im.row0 + y];
    }
    png_block_sum2(sa, sb, red);
    if (threadIdx.x != 0) return;
    const int r0 = ridx[im.elem0], r1 = i + 1 < B ? ridx[imgs[i + 1].elem0] : *nruns;
    const int tokbits = boff[r1] - boff[r0];
    const int len = 2 + (int)(((int64_t)tokbits + 10 + 7) >> 3) + 4;    // 3 block-header bits + tokens + 7 bits of end-of-block, padded
    const bool fits = len <= im.cap;
    out_len[i] = fits ? len : -1;
    if (!fits) *err = 1;
    const unsigned long long n = (unsigned long long)im.H * (unsigned long long)(im.W + 1);
    const uint32_t A = (uint32_t)((1 + sa) % kAdlerMod), Bv = (uint32_t)((n % kAdlerMod + sb) % kAdlerMod);
    const uint32_t adler = (Bv << 16) | A;
    uint32_t* w = words + im.word0;
    atomicOr(w, 0x78u | (0x01u << 8) | (0x3u << 16));   // 78 01, then BFINAL = 1, BTYPE = 01 (LSB first: 1, 1, 0)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = len - 4 + k;
        atomicOr(w + (p >> 2), ((adler >> (24 - 8 * k)) & 0xFFu) << (8 * (p & 3)));
    }
}

__global__ __launch_bounds__(256) void png_copy_kernel(const PngImage* __restrict__ imgs, int B, int nwords, const uint32_t* __restrict__ words,
                                                       const int* __restrict__ out_len, uint8_t* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nwords) return;
    const int ii = png_find_image<&PngImage::word0>(imgs, B, g);
    const PngImage im = imgs[ii];
    const int len = out_len[ii], j0 = (g - im.word0) * 4;
    if (j0 >= len) return;                              // (len is -1 for an image that does not fit)
    const uint32_t v = words[g];
    uint8_t* dst = out + im.out_off + j0;
    const int nb = min(4, len - j0);
    for (int k = 0; k < nb; k++) dst[k] = (uint8_t)(v >> (8 * k));
}

// RFC 1951 3.2.5 / 3.2.6: the fixed literal / length code, bit-reversed because Huffman codes enter the LSB-first stream from
// their most significant bit
static uint32_t png_reverse(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

static PngTables png_make_tables() {
    PngTables T{};
    for (int b = 0; b < 256; b++) T.lit[b] = (uint16_t)(b < 144 ? png_reverse(0x30 + b, 8) : png_reverse(0x190 + (b - 144), 9));
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int len = 3; len <= 258; len++) {
        int c = 28;
        while (base[c] > len) c--;                      // (258 has a code of its own; 227 .. 257 are code 284 + extra bits)
        const int sym = 257 + c;
        const int hl = sym < 280 ? 7 : 8;
        const uint32_t code = sym < 280 ? png_reverse(sym - 256, 7) : png_reverse(0xC0 + (sym - 280), 8);
        T.match[len - 3] = ((uint32_t)(hl + extra[c] + 5) << 24) | code | ((uint32_t)(len - base[c]) << hl);
    }
    return T;
}

static inline size_t png_align(size_t v) { return (v + 255) & ~(size_t)255; }

int png_encode(const uint8_t* d_labels, const pnp_png_image* h_imgs, int B, uint8_t* d_out, int* d_out_len, int* d_err, void* d_ws,
               int64_t ws_bytes, int64_t* ws_need, hipStream_t s) {
    if (!h_imgs || B < 1) return PNP_ERR_ARG;
    std::vector<PngImage> im((size_t)B);
    int64_t rows = 0, elems = 0, words = 0;
    for (int i = 0; i < B; i++) {
        const pnp_png_image& h = h_imgs[i];
        if (h.H < 1 || h.W < 1 || h.H > 65535 || h.W > 65535 || h.out_cap < 0 || h.labels_off < 0 || h.out_off < 0) return PNP_ERR_ARG;
        PngImage& e = im[(size_t)i];
        e.lab_off = h.labels_off;
        e.out_off = h.out_off;
        e.H = h.H;
        e.W = h.W;
        e.cap = h.out_cap;
        e.row0 = (int32_t)rows;
        e.elem0 = (int32_t)elems;
        e.word0 = (int32_t)words;
        const int64_t n = (int64_t)h.H * (h.W + 1);
        rows += h.H;
        elems += n;
        if (elems > kPngMaxElems) return PNP_ERR_ARG;
        words += (2 + (10 + 9 * n + 7) / 8 + 4 + 3) / 4 + 1;           // the worst case of the format (all 9-bit literals), in words
    }
    const size_t N = (size_t)elems;
    size_t o = 0;
    const size_t o_img = o;    o += png_align(sizeof(PngImage) * (size_t)B);
    const size_t o_tab = o;    o += png_align(sizeof(PngTables));
    const size_t o_filt = o;   o += png_align(N);
    const size_t o_head = o;   o += png_align((N + 1) * sizeof(int));           // run-head flags, then the runs' bit lengths
    const size_t o_ridx = o;   o += png_align(N * sizeof(int));
    const size_t o_rpos = o;   o += png_align((N + 1) * sizeof(int));
    const size_t o_boff = o;   o += png_align((N + 1) * sizeof(int));
    const size_t o_rowa = o;   o += png_align((size_t)rows * sizeof(uint32_t));
    const size_t o_rowb = o;   o += png_align((size_t)rows * sizeof(uint32_t));
    const size_t o_nrun = o;   o += png_align(sizeof(int));
    const size_t o_words = o;  o += png_align((size_t)words * sizeof(uint32_t));
    const size_t o_tmp = o;
    const size_t tmp_bytes = sort_temp_bytes(N + 1);
    o += png_align(tmp_bytes);
    if (ws_need) *ws_need = (int64_t)o;
    if (!d_ws) return ws_need ? PNP_OK : PNP_ERR_ARG;
    if (!d_labels || !d_out || !d_out_len || !d_err || ws_bytes < (int64_t)o) return PNP_ERR_ARG;

    static const PngTables tables = png_make_tables();
    uint8_t* ws = reinterpret_cast<uint8_t*>(d_ws);
    PngImage* d_img = reinterpret_cast<PngImage*>(ws + o_img);
    PngTables* d_tab = reinterpret_cast<PngTables*>(ws + o_tab);
    uint8_t* d_filt = ws + o_filt;
    int* d_head = reinterpret_cast<int*>(ws + o_head);
    int* d_nbits = d_head;
    int* d_ridx = reinterpret_cast<int*>(ws + o_ridx);
    int* d_rpos = reinterpret_cast<int*>(ws + o_rpos);
    int* d_boff = reinterpret_cast<int*>(ws + o_boff);
    uint32_t* d_rowa = reinterpret_cast<uint32_t*>(ws + o_rowa);
    uint32_t* d_rowb = reinterpret_cast<uint32_t*>(ws + o_rowb);
    int* d_nrun = reinterpret_cast<int*>(ws + o_nrun);
    uint32_t* d_words = reinterpret_cast<uint32_t*>(ws + o_words);
    if (hipMemcpyAsync(d_img, im.data(), sizeof(PngImage) * (size_t)B, hipMemcpyHostToDevice, s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemcpyAsync(d_tab, &tables, sizeof(PngTables), hipMemcpyHostToDevice, s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemsetAsync(d_words, 0, (size_t)words * sizeof(uint32_t), s) != hipSuccess) return PNP_ERR_HIP;
    if (hipMemsetAsync(d_err, 0, sizeof(int), s) != hipSuccess) return PNP_ERR_HIP;
    const int n = (int)N;
    const unsigned ge = (unsigned)((N + 255) / 256), gr = (unsigned)((N + 1 + 255) / 256), gw = (unsigned)((words + 255) / 256);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)rows), dim3(256), 0, s, d_labels, (const PngImage*)d_img, B, d_filt, d_head, d_rowa, d_rowb);
    int r = device_scan_i32(d_head, d_ridx, N, false, ws + o_tmp, tmp_bytes, s);
    if (r != PNP_OK) return r;
    hipLaunchKernelGGL(png_runs_kernel, dim3(ge), dim3(256), 0, s, (const int*)d_head, (const int*)d_ridx, n, d_rpos, d_nrun);
    hipLaunchKernelGGL(png_bits_kernel, dim3(gr), dim3(256), 0, s, (const uint8_t*)d_filt, (const int*)d_rpos, (const int*)d_nrun,
                       (const PngTables*)d_tab, n, d_nbits);
    r = device_scan_i32(d_nbits, d_boff, N + 1, false, ws + o_tmp, tmp_bytes, s);
    if (r != PNP_OK) return r;
    hipLaunchKernelGGL(png_pack_kernel, dim3(ge), dim3(256), 0, s, (const uint8_t*)d_filt, (const int*)d_rpos, (const int*)d_nrun,
                       (const int*)d_ridx, (const int*)d_boff, (const PngImage*)d_img, B, (const PngTables*)d_tab, d_words);
    hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, (const PngImage*)d_img, B, (const int*)d_nrun, (const int*)d_ridx,
                       (const int*)d_boff, (const uint32_t*)d_rowa, (const uint32_t*)d_rowb, d_words, d_out_len, d_err);
    hipLaunchKernelGGL(png_copy_kernel, dim3(gw), dim3(256), 0, s, (const PngImage*)d_img, B, (int)words, (const uint32_t*)d_words,
                       (const int*)d_out_len, d_out);
    return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP;
}

}  // namespace pnp

extern "C" int pnp_png_encode(const uint8_t* d_labels, const pnp_png_image* h_images, int32_t n_images, uint8_t* d_out, int32_t* d_out_len,
                              int32_t* d_err, void* d_ws, int64_t ws_bytes, int64_t* ws_need, void* stream) {
    return pnp::png_encode(d_labels, h_images, n_images, d_out, d_out_len, d_err, d_ws, ws_bytes, ws_need, (hipStream_t)stream);
}
