// Progressive JPEG (SOF2) entropy decode on gfx950, scan by scan, in front of the coefficient buffers, inverse DCT and
// colour kernels of jpeg.hip.  The host (pnp_ovss/jpeg.py pack_scans) records every scan of every file and checks the
// progression; the device restates T.81 G.1.2, one workgroup of 1024 threads per restart segment of a scan, one launch per
// (scan ordinal, scan kind) over the segments of every image's scan of that ordinal, so a file's scans run in file order:
//   jpeg_dc_refine_kernel          no Huffman code: bit n of the segment is bit Al of the DC of block n
//   jpeg_scan_kernel<DC_FIRST>     a Huffman symbol + magnitude bits per block, (pred + diff) << Al; state (bit, block-in-MCU)
//   jpeg_scan_kernel<AC_FIRST>     run / size symbols of one band Ss..Se of one component, values << Al; an end-of-band run
//                                  EOBn covers 2^n + n more bits blocks and consumes no further bits, so it only advances
//                                  the block count: state (bit, zig-zag index)
//   jpeg_scan_kernel<AC_REFINE>    each newly non-zero coefficient is +-(1 << Al); zero runs count only positions whose value
//                                  BEFORE this scan is zero, and every position with history passed over -- inside an
//                                  end-of-band run too -- is followed by one correction bit.  What a symbol consumes depends
//                                  on the block it stands in: state (bit, absolute block, zig-zag index, blocks left in run)
// The three Huffman kinds use the sub-sequence scheme of jpeg_huffman_kernel: the segment is cut into up to 1024 pieces of equal
// bit length, thread i decodes piece i from a guessed entry state and takes over the exit state of thread i - 1 until no entry
// state changes -- the fixed point of S[i + 1] = f(S[i]) with S[0] exact is the sequential decode.  These rounds write nothing.
// Block counts (and DC sums) per piece are prefix-summed, then one pass writes.  For AC refinement the rounds read the
// scan's history as one 64-bit mask per block (bit k: zig-zag coefficient k is non-zero), which the workgroup computes from the
// coefficients before the first round; the writing pass reads and corrects only positions at or behind its own entry state,
// which no earlier piece writes.
#include "common.h"
#include "kernels.h"

namespace pnp {
namespace {

__constant__ int kProgZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int PROG_T = 1024;          // threads = sub-sequences per segment
constexpr int PROG_LA = 10;           // look-ahead bits of the code tables
constexpr int PROG_MAXB = 6;          // blocks per MCU (4:2:0)
enum { DC_FIRST = 1, DC_REFINE = 2, AC_FIRST = 3, AC_REFINE = 4 };

struct ProgLds {
    uint16_t fast[4][1 << PROG_LA];
    int mincode[4][17], maxcode[4][17], valptr[4][17];
    uint8_t vals[4][256];
    int zz[64];
    // per block of the scan's unit: component, table slot (DC or AC, whichever the scan codes), position in the MCU, and the
    // component's sampling factors, plane width in blocks and coefficient offset (1 x 1 factors for a one-component scan)
    int mb_c[PROG_MAXB], mb_t[PROG_MAXB], mb_by[PROG_MAXB], mb_bx[PROG_MAXB], mb_h[PROG_MAXB], mb_v[PROG_MAXB], mb_bxc[PROG_MAXB];
    long mb_coef[PROG_MAXB];
    unsigned Ep[PROG_T];
    int Ea[PROG_T], Eb[PROG_T], Ec[PROG_T], Edc[3][PROG_T];
    int wsum[PROG_T / 64];
    int done;
};

struct ProgGeom {            // uniform per workgroup
    int bpm, ux, unit0, total_blocks, ss, se, al, maxw;
};

struct ProgState {
    unsigned p;              // bit position
    int a;                   // DC first: block in the MCU; AC: zig-zag index
    int b;                   // block of the segment (AC refinement: part of the state; else counted from the entry)
    int c;                   // AC refinement: blocks left in the end-of-band run
};

__device__ __forceinline__ int prog_excl_scan(int v, int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w && i < nw; i++) off += wsum[i];
    return off + x - v;
}

// big-endian bit reader over the un-stuffed words of a segment; never reads behind word `maxw` (the zero tail the
// un-stuffing kernel wrote up to clean_cap)
struct ProgBits {
    const uint32_t* w;
    uint32_t wp, maxw;
    uint64_t acc;
    int nb;
    unsigned p;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return __builtin_bswap32(w[i < maxw ? i : maxw]); }
    __device__ __forceinline__ void open(const uint32_t* words, unsigned pos, int max_word) {
        w = words;
        maxw = (uint32_t)max_word;
        p = pos;
        wp = pos >> 5;
        acc = (((uint64_t)word(wp) << 32) | word(wp + 1)) << (pos & 31);
        nb = 64 - (pos & 31);
        wp += 2;
    }
    __device__ __forceinline__ void fill() {             // afterwards at least 32 valid bits
        if (nb < 32) {
            acc |= (uint64_t)word(wp) << (32 - nb);
            nb += 32;
            wp++;
        }
    }
    __device__ __forceinline__ unsigned peek16() const { return (unsigned)(acc >> 48); }
    __device__ __forceinline__ void skip(int n) {        // n <= 32, after fill()
        acc <<= n;
        nb -= n;
        p += n;
    }
    __device__ __forceinline__ unsigned take(int n) {    // n <= 16, after fill() and at most 16 bits taken since
        const unsigned v = n ? (unsigned)(acc >> (64 - n)) : 0u;
        skip(n);
        return v;
    }
    __device__ __forceinline__ void skip_many(int n) {
        while (n > 0) {
            fill();
            const int m = n < 32 ? n : 32;
            skip(m);
            n -= m;
        }
    }
};

// one Huffman symbol of table t (T.81 F.2.2.3); consumes its code.  bad: no code of any length matches
__device__ __forceinline__ int prog_symbol(const ProgLds& S, int t, ProgBits& br, bool& bad) {
    const unsigned top = br.peek16();
    const unsigned f = S.fast[t][top >> (16 - PROG_LA)];
    int len = f >> 8, sym = f & 255;
    if (len == 0) {
        len = 16;
        sym = 0;
        bad = true;
        for (int l = PROG_LA + 1; l <= 16; l++) {
            const int code = (int)(top >> (16 - l));
            if (S.maxcode[t][l] >= 0 && code <= S.maxcode[t][l] && code >= S.mincode[t][l]) {
                len = l;
                sym = S.vals[t][(S.valptr[t][l] + code - S.mincode[t][l]) & 255];
                bad = false;
                break;
            }
        }
    }
    br.skip(len);
    return sym;
}

__device__ __forceinline__ int prog_extend(unsigned vb, int s) { return (s == 0 || vb >= (1u << (s - 1))) ? (int)vb : (int)vb - (1 << s) + 1; }

// element offset of block n of the segment (bi: its position in the unit) in the coefficient buffer
__device__ __forceinline__ long prog_block(const ProgLds& S, const ProgGeom& G, int n, int bi) {
    const int unit = G.unit0 + n / G.bpm;
    const int uy = unit / G.ux, ux = unit - uy * G.ux;
    return S.mb_coef[bi] + ((long)(uy * S.mb_v[bi] + S.mb_by[bi]) * S.mb_bxc[bi] + (ux * S.mb_h[bi] + S.mb_bx[bi])) * 64;
}

// tables, zig-zag order and the scan's geometry into LDS.  false: descriptors the host never writes (the caller reports them)
__device__ bool prog_setup(ProgLds& S, ProgGeom& G, const JpegImage* ip, const JpegScan& sc, const JpegSegment& sg, const JpegTables& T) {
    const int tid = threadIdx.x;
    if (tid < 4) {
        int code = 0, kk = 0;
        for (int l = 1; l <= 16; l++) {
            const int cnt = T.counts[tid][l - 1];
            S.valptr[tid][l] = kk;
            S.mincode[tid][l] = code;
            code += cnt;
            kk += cnt;
            S.maxcode[tid][l] = cnt ? code - 1 : -1;
            code <<= 1;
        }
    }
    for (int i = tid; i < 4 * 256; i += blockDim.x) (&S.vals[0][0])[i] = (&T.vals[0][0])[i];
    if (tid < 64) S.zz[tid] = kProgZigzag[tid];
    const bool single = sc.ncomp == 1;
    int bpm = 0;
    bool ok = sc.ncomp >= 1 && sc.ncomp <= 3 && sc.ss >= 0 && sc.ss <= sc.se && sc.se <= 63 && sc.al >= 0 && sc.al <= 13 && sc.bw > 0;
    for (int q = 0; ok && q < sc.ncomp; q++) {
        const int c = sc.comp[q];
        if (c < 0 || c >= ip->ncomp || c > 2) {
            ok = false;
            break;
        }
        const int hc = single ? 1 : ip->h[c], vc = single ? 1 : ip->v[c];
        if (hc < 1 || vc < 1 || bpm + hc * vc > PROG_MAXB) {
            ok = false;
            break;
        }
        if (tid == 0)
            for (int y = 0; y < vc; y++)
                for (int x = 0; x < hc; x++) {
                    const int bi = bpm + y * hc + x;
                    S.mb_c[bi] = c;
                    S.mb_t[bi] = sc.ss == 0 ? (sc.td[q] & 1) : 2 + (sc.ta[q] & 1);
                    S.mb_by[bi] = y;
                    S.mb_bx[bi] = x;
                    S.mb_h[bi] = hc;
                    S.mb_v[bi] = vc;
                    S.mb_bxc[bi] = ip->bx[c];
                    S.mb_coef[bi] = ip->coef_off[c];
                }
        bpm += hc * vc;
    }
    if (ok && single) {                                   // the scan's own grid must lie inside the component's plane
        const int c = sc.comp[0];
        ok = sc.bw <= ip->bx[c] && sc.bh <= ip->by[c];
    } else if (ok) {
        ok = sc.bw == ip->mcux && sc.bh == ip->mcuy;
    }
    ok = ok && sg.mcu0 >= 0 && sg.nmcu >= 0 && (long)sg.mcu0 + sg.nmcu <= (long)sc.bw * sc.bh;
    G.bpm = bpm;
    G.ux = sc.bw;
    G.unit0 = sg.mcu0;
    G.total_blocks = ok ? sg.nmcu * bpm : 0;
    G.ss = sc.ss;
    G.se = sc.se;
    G.al = sc.al;
    G.maxw = sg.clean_cap / 4 - 1;
    __syncthreads();
    for (int i = tid; i < 4 << PROG_LA; i += blockDim.x) {
        const int t = i >> PROG_LA, x = i & ((1 << PROG_LA) - 1);
        unsigned e = 0;
        for (int l = 1; l <= PROG_LA; l++) {
            const int code = x >> (PROG_LA - l);
            if (S.maxcode[t][l] >= 0 && code <= S.maxcode[t][l] && code >= S.mincode[t][l]) {
                e = ((unsigned)l << 8) | S.vals[t][(S.valptr[t][l] + code - S.mincode[t][l]) & 255];
                break;
            }
        }
        S.fast[t][x] = (uint16_t)e;
    }
    if (tid == 0) S.done = 0;
    __syncthreads();
    return ok;
}

__device__ __forceinline__ uint64_t bits_from(int k) { return k > 63 ? 0ull : ~0ull << k; }

// Decode from state st up to the first code boundary at or behind p_end (or the segment's last block).  WRITE = false: only
// the exit state, the blocks completed (st.b) and the DC sums (the synchronisation rounds).  WRITE = true: st.b is the absolute
// block, d0..d2 the DC predictors at the entry; coefficients go to global memory and errors are reported.
template <int KIND, bool WRITE>
__device__ __forceinline__ void prog_run(const ProgLds& S, const ProgGeom& G, const uint32_t* __restrict__ words, ProgState& st,
                                         unsigned p_end, int& d0, int& d1, int& d2, int16_t* __restrict__ coef,
                                         const uint64_t* __restrict__ hist, int* __restrict__ err, int* done) {
    ProgBits br;
    br.open(words, st.p, G.maxw);
    const int p1 = 1 << G.al;
    const uint64_t band = bits_from(G.ss) & (~0ull >> (63 - G.se));
    while (!(WRITE || KIND == AC_REFINE) || st.b < G.total_blocks) {
        if (br.p >= p_end) {
            // behind the last bit of the piece only what needs no bit goes on: the blocks of an end-of-band run of a refinement
            // scan that have no history left in the band (the run may outlast the segment's bits, padding apart)
            if (KIND != AC_REFINE || st.c == 0) break;
            if (hist[prog_block(S, G, st.b, 0) >> 6] & band & bits_from(st.a)) break;
        }
        br.fill();
        bool bad = false;
        if (KIND == DC_FIRST) {
            const int c = S.mb_c[st.a];
            const int sym = prog_symbol(S, S.mb_t[st.a], br, bad);
            const int s = sym & 15;
            if (WRITE && (bad || sym > 11)) atomicExch(err, 1);
            const int v = prog_extend(br.take(s), s);
            d0 += c == 0 ? v : 0;
            d1 += c == 1 ? v : 0;
            d2 += c == 2 ? v : 0;
            if (WRITE) coef[prog_block(S, G, st.b, st.a)] = (int16_t)((c == 0 ? d0 : (c == 1 ? d1 : d2)) * p1);
            st.a = st.a + 1 == G.bpm ? 0 : st.a + 1;
            st.b++;
        } else if (KIND == AC_FIRST) {
            const int sym = prog_symbol(S, S.mb_t[0], br, bad);
            const int r = sym >> 4, s = sym & 15;
            if (WRITE && bad) atomicExch(err, 1);
            if (s) {
                st.a += r;
                const int v = prog_extend(br.take(s), s);
                if (st.a > G.se) {
                    if (WRITE) atomicExch(err, 1);
                } else if (WRITE) {
                    coef[prog_block(S, G, st.b, 0) + S.zz[st.a]] = (int16_t)(v * p1);
                }
                st.a++;
            } else if (r == 15) {
                st.a += 16;
                if (WRITE && st.a > G.se) atomicExch(err, 1);
            } else {                                          // end-of-band run: this block and run - 1 more
                const int run = (1 << r) + (int)br.take(r);
                if (WRITE && run > G.total_blocks - st.b) atomicExch(err, 1);
                st.b += run;
                st.a = G.ss;
            }
            if (st.a > G.se) {
                st.a = G.ss;
                st.b++;
            }
        } else {                                              // AC_REFINE
            const long off = prog_block(S, G, st.b, 0);
            const uint64_t M = hist[off >> 6] & band;
            // one correction bit behind every position of C, in zig-zag order
            auto correct = [&](uint64_t C) {
                if (!WRITE) {
                    br.skip_many(__popcll(C));
                    return;
                }
                while (C) {
                    const int j = __ffsll((long long)C) - 1;
                    C &= C - 1;
                    br.fill();
                    if (br.take(1)) {
                        int16_t* q = coef + off + S.zz[j];
                        const int v = *q;
                        if ((v & p1) == 0) *q = (int16_t)(v >= 0 ? v + p1 : v - p1);
                    }
                }
            };
            if (st.c == 0) {
                const int sym = prog_symbol(S, S.mb_t[0], br, bad);
                const int r = sym >> 4, s = sym & 15;
                if (WRITE && (bad || s > 1)) atomicExch(err, 1);
                if (s == 0 && r < 15) {
                    st.c = (1 << r) + (int)br.take(r);
                    if (WRITE && st.c > G.total_blocks - st.b) atomicExch(err, 1);
                } else {
                    const unsigned positive = s ? br.take(1) : 0u;
                    uint64_t Z = ~M & bits_from(st.a) & band;      // history-zero positions still ahead in this block
                    for (int i = 0; i < r; i++) Z &= Z - 1;        // r of them are passed; the next one is the target
                    if (Z == 0) {                                  // the run leaves the band
                        correct(M & bits_from(st.a));
                        if (WRITE) atomicExch(err, 1);
                        st.a = G.se + 1;
                    } else {
                        const int t = __ffsll((long long)Z) - 1;
                        correct(M & bits_from(st.a) & ~bits_from(t));
                        if (WRITE && s) coef[off + S.zz[t]] = (int16_t)(positive ? p1 : -p1);
                        st.a = t + 1;
                    }
                }
            }
            if (st.c > 0) {                                        // the rest of this block lies inside an end-of-band run
                correct(M & bits_from(st.a));
                st.c--;
                st.a = G.se + 1;
            }
            if (st.a > G.se) {
                st.a = G.ss;
                st.b++;
            }
        }
    }
    st.p = br.p;
    if (WRITE && st.b >= G.total_blocks) *done = 1;
}

template <int KIND>
__global__ __launch_bounds__(PROG_T) void jpeg_scan_kernel(const uint8_t* __restrict__ clean, const JpegImage* __restrict__ imgs,
                                                           const JpegTables* __restrict__ tabs, const JpegScan* __restrict__ scans,
                                                           const JpegSegment* __restrict__ segs, const int* __restrict__ seg_bits,
                                                           int first, int16_t* __restrict__ coef, uint64_t* __restrict__ hist,
                                                           int* __restrict__ rounds, int* __restrict__ err) {
    __shared__ ProgLds S;
    const int si = first + blockIdx.x;
    const JpegSegment sg = segs[si];
    const JpegScan& sc = scans[sg.scan];
    const JpegImage* const ip = imgs + sg.image;
    const int tid = threadIdx.x;
    ProgGeom G;
    const bool ok = prog_setup(S, G, ip, sc, sg, tabs[sc.tab]);
    if (!ok || sc.kind != KIND || (KIND != DC_FIRST && sc.ncomp != 1)) {
        if (tid == 0) {
            atomicExch(err, 1);
            if (rounds) rounds[si] = 0;
        }
        return;
    }
    if (KIND == AC_REFINE) {                              // the history of every block of the segment, before anything is written
        for (int n = tid; n < G.total_blocks; n += PROG_T) {
            const long off = prog_block(S, G, n, 0);
            uint64_t m = 0;
#pragma unroll 8
            for (int k = 1; k < 64; k++) m |= (uint64_t)(coef[off + S.zz[k]] != 0) << k;
            hist[off >> 6] = m;
        }
        __syncthreads();
    }
    const uint32_t* words = reinterpret_cast<const uint32_t*>(clean + sg.clean_off);
    const unsigned total_bits = (unsigned)seg_bits[si];
    const unsigned sub = (unsigned)sg.sub_bits;
    const int nsub = (int)min((total_bits + sub - 1) / sub, (unsigned)PROG_T);
    const bool live = tid < nsub;
    const unsigned p_end = live ? (tid == nsub - 1 ? total_bits : (unsigned)(tid + 1) * sub) : 0u;
    // entry state: exact for thread 0, a guess (a block starts at the cut; AC refinement: at the same fraction of the blocks)
    ProgState e;
    e.p = (unsigned)tid * sub;
    e.a = KIND == DC_FIRST ? 0 : G.ss;
    e.b = KIND == AC_REFINE && tid > 0 && total_bits ? (int)((uint64_t)e.p * G.total_blocks / total_bits) : 0;
    e.c = 0;
    if (KIND == AC_REFINE && e.b >= G.total_blocks) e.b = G.total_blocks > 0 ? G.total_blocks - 1 : 0;
    bool dirty = live;
    int taken = 0;
    for (int round = 0; round <= PROG_T; round++) {
        if (dirty) {
            ProgState st = e;
            if (KIND != AC_REFINE) st.b = 0;
            int d0 = 0, d1 = 0, d2 = 0;
            prog_run<KIND, false>(S, G, words, st, p_end, d0, d1, d2, nullptr, hist, nullptr, nullptr);
            S.Ep[tid] = st.p;
            S.Ea[tid] = st.a;
            S.Eb[tid] = st.b;
            S.Ec[tid] = st.c;
            S.Edc[0][tid] = d0;
            S.Edc[1][tid] = d1;
            S.Edc[2][tid] = d2;
        }
        __syncthreads();
        dirty = false;
        if (live && tid > 0) {
            const unsigned np = S.Ep[tid - 1];
            const int na = S.Ea[tid - 1], nb = S.Eb[tid - 1], nc = S.Ec[tid - 1];
            if (np != e.p || na != e.a || (KIND == AC_REFINE && (nb != e.b || nc != e.c))) {
                e.p = np;
                e.a = na;
                if (KIND == AC_REFINE) {
                    e.b = nb;
                    e.c = nc;
                }
                dirty = true;
            }
        }
        taken = round + 1;
        if (!__syncthreads_or(dirty ? 1 : 0)) break;
    }
    if (tid == 0 && rounds) rounds[si] = taken;
    // absolute block and DC predictors at every entry state, then the writing pass
    int d0 = 0, d1 = 0, d2 = 0;
    if (KIND != AC_REFINE) e.b = prog_excl_scan(live ? S.Eb[tid] : 0, S.wsum);
    if (KIND == DC_FIRST) {
        d0 = prog_excl_scan(live ? S.Edc[0][tid] : 0, S.wsum);
        d1 = prog_excl_scan(live ? S.Edc[1][tid] : 0, S.wsum);
        d2 = prog_excl_scan(live ? S.Edc[2][tid] : 0, S.wsum);
    }
    if (live && e.b >= 0 && e.b < G.total_blocks && e.p < total_bits) {
        if (KIND == DC_FIRST && e.a != e.b % G.bpm) atomicExch(err, 1);
        ProgState st = e;
        prog_run<KIND, true>(S, G, words, st, p_end, d0, d1, d2, coef, hist, err, &S.done);
    }
    __syncthreads();
    if (tid == 0 && !S.done && G.total_blocks > 0) atomicExch(err, 1);       // the stream ended before the last block
}

__global__ __launch_bounds__(PROG_T) void jpeg_dc_refine_kernel(const uint8_t* __restrict__ clean, const JpegImage* __restrict__ imgs,
                                                                const JpegTables* __restrict__ tabs, const JpegScan* __restrict__ scans,
                                                                const JpegSegment* __restrict__ segs, const int* __restrict__ seg_bits,
                                                                int first, int16_t* __restrict__ coef, int* __restrict__ rounds,
                                                                int* __restrict__ err) {
    __shared__ ProgLds S;
    const int si = first + blockIdx.x;
    const JpegSegment sg = segs[si];
    const JpegScan& sc = scans[sg.scan];
    ProgGeom G;
    const bool ok = prog_setup(S, G, imgs + sg.image, sc, sg, tabs[sc.tab]);
    const int tid = threadIdx.x;
    if (tid == 0 && rounds) rounds[si] = 0;
    if (!ok || sc.kind != DC_REFINE || sc.ss != 0 || (unsigned)seg_bits[si] < (unsigned)G.total_blocks) {
        if (tid == 0) atomicExch(err, 1);                 // (a stream shorter than one bit per block ended early)
        return;
    }
    const uint32_t* words = reinterpret_cast<const uint32_t*>(clean + sg.clean_off);
    for (int n = tid; n < G.total_blocks; n += PROG_T) {
        const uint32_t w = __builtin_bswap32(words[n >> 5]);
        if (w >> (31 - (n & 31)) & 1) {
            int16_t* q = coef + prog_block(S, G, n, n % G.bpm);
            *q = (int16_t)(*q | (1 << G.al));
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------ host
int jpeg_decode_scans(const uint8_t* d_data, const JpegImage* d_imgs, const JpegTables* d_tabs, const JpegScan* d_scans,
                      const JpegSegment* d_segs, int n_images, int n_segments, int n_base_segments, const int32_t* h_groups, int n_groups,
                      uint8_t* d_clean, int* d_seg_bits, int16_t* d_coef, size_t coef_elems, uint64_t* d_hist, uint8_t* d_planes,
                      uint8_t* d_rgb, int max_blocks, int max_pixels, int* d_rounds, float* h_group_ms, int* d_err, hipStream_t s) {
    if (hipMemsetAsync(d_coef, 0, coef_elems * sizeof(int16_t), s) != hipSuccess) return PNP_ERR_HIP;
    jpeg_launch_unstuff(d_data, d_imgs, d_segs, n_segments, d_clean, d_seg_bits, s);
    if (n_base_segments > 0) {
        jpeg_launch_huffman(d_clean, d_imgs, d_tabs, d_segs, n_base_segments, d_seg_bits, d_coef, d_err, s);
        if (d_rounds && hipMemsetAsync(d_rounds, 0, (size_t)n_base_segments * sizeof(int), s) != hipSuccess) return PNP_ERR_HIP;
    }
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (h_group_ms && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) return PNP_ERR_HIP;
    int rc = PNP_OK;
    for (int g = 0; g < n_groups && rc == PNP_OK; g++) {
        const int first = h_groups[4 * g], count = h_groups[4 * g + 1], kind = h_groups[4 * g + 2];
        if (h_group_ms) (void)hipEventRecord(ev[0], s);
        const dim3 grid(count), block(PROG_T);
        if (kind == DC_FIRST)
            hipLaunchKernelGGL(jpeg_scan_kernel<DC_FIRST>, grid, block, 0, s, d_clean, d_imgs, d_tabs, d_scans, d_segs, d_seg_bits, first, d_coef,
                               d_hist, d_rounds, d_err);
        else if (kind == AC_FIRST)
            hipLaunchKernelGGL(jpeg_scan_kernel<AC_FIRST>, grid, block, 0, s, d_clean, d_imgs, d_tabs, d_scans, d_segs, d_seg_bits, first, d_coef,
                               d_hist, d_rounds, d_err);
        else if (kind == AC_REFINE)
            hipLaunchKernelGGL(jpeg_scan_kernel<AC_REFINE>, grid, block, 0, s, d_clean, d_imgs, d_tabs, d_scans, d_segs, d_seg_bits, first, d_coef,
                               d_hist, d_rounds, d_err);
        else
            hipLaunchKernelGGL(jpeg_dc_refine_kernel, grid, block, 0, s, d_clean, d_imgs, d_tabs, d_scans, d_segs, d_seg_bits, first, d_coef,
                               d_rounds, d_err);
        if (h_group_ms) {                                 // profiling: one launch at a time between two events
            (void)hipEventRecord(ev[1], s);
            if (hipEventSynchronize(ev[1]) != hipSuccess || hipEventElapsedTime(&h_group_ms[g], ev[0], ev[1]) != hipSuccess) rc = PNP_ERR_HIP;
        }
    }
    if (h_group_ms) {
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    if (rc != PNP_OK) return rc;
    jpeg_launch_pixels(d_imgs, d_tabs, n_images, d_coef, d_planes, d_rgb, max_blocks, max_pixels, s);
    return hipGetLastError() == hipSuccess ? PNP_OK : PNP_ERR_HIP;
}

}  // namespace pnp
