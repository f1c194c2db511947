"""Progressive (SOF2) JPEG streams for the decoder tests (test_jpeg_progressive_cpu.py, test_jpeg_progressive_gpu.py): a writer
for arbitrary scan scripts and a pure-Python reference decoder over the packed descriptors, both restating T.81 Annex G in
plain Python, independent of the code under test.

`recode_progressive` takes the quantised coefficients of a baseline stream Pillow encoded (`_jpeg_streams.quantised`) and
writes them as a SOF2 file for any legal scan script; Pillow decodes the result to the pixels of the source, which
test_jpeg_progressive_cpu.py asserts for every script.  `decode_packed` walks the arrays `pnp_ovss.jpeg.pack_scans` hands to
the device -- images, tables, scans, segments -- and returns the coefficient planes.

A script is a list of scans (components, Ss, Se, Ah, Al), components being indices into the frame."""
import functools

import numpy as np

import _jpeg_streams as S
from oracle import jpeg_np as J

ZZ = [int(z) for z in J.ZIGZAG]

# One legal table per class that holds every symbol a progressive scan can need.  AC: all (run, size <= 10) pairs, 176
# symbols -- EOBn is (n, 0), ZRL (15, 0) -- at lengths 2..12, so short codes, codes of the look-ahead length and longer ones
# all occur.  Two orders of the same symbols, so that two table ids hold different tables.
_AC_COUNTS = [0, 1, 1, 1, 2, 4, 8, 16, 32, 50, 0, 61, 0, 0, 0, 0]
_AC_FIRST = [0x01, 0x00, 0x11, 0x02, 0x21, 0x10, 0x31, 0x03, 0x41, 0x12, 0x20, 0x51, 0x04, 0x61, 0x30, 0xF0]
_AC_ALL = [r << 4 | s for r in range(16) for s in range(11)]
PROG_AC = (_AC_COUNTS, _AC_FIRST + [s for s in _AC_ALL if s not in _AC_FIRST])
PROG_AC_B = (_AC_COUNTS, _AC_FIRST[::-1] + [s for s in reversed(_AC_ALL) if s not in _AC_FIRST])
PROG_DC = S.STD_DC
PROG_DC_B = S.UNARY_DC
for _t in (PROG_AC, PROG_AC_B, PROG_DC, PROG_DC_B):
    S.check_tables_legal(*_t)


# ------------------------------------------------------------------------------------------ scan scripts
def pillow_script(nc):
    """libjpeg's jpeg_simple_progression: 10 scans for YCbCr, 6 for greyscale."""
    if nc == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
            ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def _all(nc):
    return tuple(range(nc))


def spectral_script(nc):
    """Spectral selection only: DC, then bands 1-5 and 6-63 per component, all Ah = Al = 0."""
    return [(_all(nc), 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in range(nc) for a, b in ((1, 5), (6, 63))]


def single_bands_script(nc):
    """One band per coefficient for the first 8, the rest in one band."""
    return [(_all(nc), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(nc) for k in range(1, 9)] + [((c,), 9, 63, 0, 0) for c in range(nc)]


def approximation_script(nc):
    """Successive approximation from Al = 3 down to 0, for DC and for the whole AC band."""
    out = [(_all(nc), 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in range(nc)]
    for al in (2, 1, 0):
        out += [(_all(nc), 0, 0, al + 1, al)] + [((c,), 1, 63, al + 1, al) for c in range(nc)]
    return out


def chroma_first_script(nc):
    """Chroma AC scans (first and refinement) before any luma AC scan."""
    order = list(range(nc))[::-1]
    return [(_all(nc), 0, 0, 0, 0)] + [((c,), 1, 63, 0, 1) for c in order] + [((c,), 1, 63, 1, 0) for c in order]


SCRIPTS = {"pillow": pillow_script, "spectral": spectral_script, "single_bands": single_bands_script,
           "approximation": approximation_script, "chroma_first": chroma_first_script}


# ------------------------------------------------------------------------------------------ the writer
PAD_BITS = {}         # stream -> per scan the number of padding bits behind its last code (0: the scan ends on a byte boundary)


def _scan_blocks(frame, comps):
    """The blocks of one scan in coding order as a list of units, each a list of (component, block row, block column); an
    interleaved scan's unit is an MCU of the padded grid, a one-component scan's unit one block of the component's own
    ceil(Xc / 8) x ceil(Yc / 8) grid."""
    hmax, vmax, mcux, mcuy = J.geometry(frame)
    cs = frame["comps"]
    if len(comps) > 1:
        return [[(c, my * cs[c]["v"] + y, mx * cs[c]["h"] + x) for c in comps for y in range(cs[c]["v"]) for x in range(cs[c]["h"])]
                for my in range(mcuy) for mx in range(mcux)]
    c = comps[0]
    bw = -(-(-(-frame["W"] * cs[c]["h"] // hmax)) // 8)
    bh = -(-(-(-frame["H"] * cs[c]["v"] // vmax)) // 8)
    return [[(c, y, x)] for y in range(bh) for x in range(bw)]


class _ScanWriter:
    """Entropy coder of one scan (T.81 G.1.2): DC first / refinement, AC first / refinement with end-of-band runs."""

    def __init__(self, dc_codes, ac_codes, Ss, Se, Ah, Al, ncomp_frame):
        self.w = S._BitWriter()
        self.dc, self.ac, self.Ss, self.Se, self.Ah, self.Al = dc_codes, ac_codes, Ss, Se, Ah, Al
        self.nc = ncomp_frame
        self.reset()

    def reset(self):
        self.pred = [0] * self.nc
        self.eobrun, self.pending = 0, []

    def flush_eobrun(self, ac):
        if self.eobrun:
            n = self.eobrun.bit_length() - 1
            self.w.put(*ac[n << 4])
            if n:
                self.w.put(self.eobrun & ((1 << n) - 1), n)
            self.eobrun = 0
        for b in self.pending:
            self.w.put(b, 1)
        self.pending = []

    def block(self, c, z):
        """z: the block's 64 coefficients in zig-zag order."""
        Ss, Se, Ah, Al, w = self.Ss, self.Se, self.Ah, self.Al, self.w
        if Ss == 0:
            if Ah:
                w.put((z[0] >> Al) & 1, 1)
                return
            v = z[0] >> Al                                    # arithmetic shift: the point transform of DC values
            d = v - self.pred[c]
            self.pred[c] = v
            s = abs(d).bit_length()
            w.put(*self.dc[c][s])
            S._magnitude(w, d, s)
            return
        ac = self.ac[c]
        a = [abs(v) >> Al for v in z]                         # AC: division towards zero
        if Ah == 0:
            run = 0
            for k in range(Ss, Se + 1):
                if a[k] == 0:
                    run += 1
                    continue
                self.flush_eobrun(ac)
                while run > 15:
                    w.put(*ac[0xF0])
                    run -= 16
                s = a[k].bit_length()
                w.put(*ac[run << 4 | s])
                S._magnitude(w, a[k] if z[k] > 0 else -a[k], s)
                run = 0
            if run:
                self.eobrun += 1
                if self.eobrun == 0x7FFF:
                    self.flush_eobrun(ac)
            return
        last_new = max([k for k in range(Ss, Se + 1) if a[k] == 1] or [-1])
        run, corr = 0, []
        for k in range(Ss, Se + 1):
            if a[k] == 0:
                run += 1
                continue
            while run > 15 and k <= last_new:
                self.flush_eobrun(ac)
                w.put(*ac[0xF0])
                run -= 16
                for b in corr:
                    w.put(b, 1)
                corr = []
            if a[k] > 1:
                corr.append(a[k] & 1)
                continue
            self.flush_eobrun(ac)
            w.put(*ac[run << 4 | 1])
            w.put(1 if z[k] > 0 else 0, 1)
            for b in corr:
                w.put(b, 1)
            run, corr = 0, []
        if run or corr:
            self.eobrun += 1
            self.pending += corr
            if self.eobrun == 0x7FFF:
                self.flush_eobrun(ac)


def recode_progressive(src, script, dri=0, dc_interleaved=True, table_ids=None, one_dht=False):
    """Write the coefficients of the baseline stream `src` as a SOF2 file with the scans of `script`.
    dri: restart interval (MCUs in an interleaved scan, blocks in a one-component scan); dc_interleaved=False: every DC scan
    of several components becomes one scan per component; table_ids: ((DC id per component), (AC id per component)), default
    luma 0 / chroma 1; one_dht: every table in ONE DHT segment in front of the first scan (else each scan brings the tables it
    uses, as libjpeg's optimised progressive files do)."""
    j, q = S.quantised(src)
    frame = j["frame"]
    cs = frame["comps"]
    nc = len(cs)
    if table_ids is None:
        table_ids = ((0, 1, 1)[:nc], (0, 1, 1)[:nc])
    dct = {t: (PROG_DC, PROG_DC_B)[t & 1] for t in set(table_ids[0])}
    act = {t: (PROG_AC, PROG_AC_B)[t & 1] for t in set(table_ids[1])}
    dcc = [S._codes(*dct[table_ids[0][c]]) for c in range(nc)]
    acc = [S._codes(*act[table_ids[1][c]]) for c in range(nc)]
    if not dc_interleaved:
        script = [s2 for s in script for s2 in ([((c,),) + tuple(s[1:]) for c in s[0]] if s[1] == 0 and len(s[0]) > 1 else [s])]

    def dht(items):
        return S._segment(0xC4, b"".join(bytes((tc << 4 | th,)) + bytes(t[0]) + bytes(t[1]) for tc, th, t in items))
    out = [b"\xff\xd8", S.JFIF]
    for t, qq in j["qt"].items():
        out.append(S._segment(0xDB, bytes((t,)) + bytes(int(x) for x in qq[J.ZIGZAG])))
    sof = bytes((8,)) + frame["H"].to_bytes(2, "big") + frame["W"].to_bytes(2, "big") + bytes((nc,))
    for c in cs:
        sof += bytes((c["id"], c["h"] << 4 | c["v"], c["tq"]))
    out.append(S._segment(0xC2, sof))
    if dri:
        out.append(S._segment(0xDD, dri.to_bytes(2, "big")))
    if one_dht:
        out.append(dht([(0, t, v) for t, v in sorted(dct.items())] + [(1, t, v) for t, v in sorted(act.items())]))
    pads = []
    zz = [[[[int(v) for v in q[c][y, x][J.ZIGZAG]] for x in range(q[c].shape[1])] for y in range(q[c].shape[0])] for c in range(nc)]
    for comps, Ss, Se, Ah, Al in script:
        if not one_dht:
            if Ss == 0 and Ah == 0:
                out += [dht([(0, t, dct[t])]) for t in sorted({table_ids[0][c] for c in comps})]
            elif Ss:
                out += [dht([(1, t, act[t])]) for t in sorted({table_ids[1][c] for c in comps})]
        sos = bytes((len(comps),)) + b"".join(bytes((cs[c]["id"], table_ids[0][c] << 4 | table_ids[1][c])) for c in comps)
        out.append(S._segment(0xDA, sos + bytes((Ss, Se, Ah << 4 | Al))))
        sw = _ScanWriter(dcc, acc, Ss, Se, Ah, Al, nc)
        rst = 0
        for n, unit in enumerate(_scan_blocks(frame, comps)):
            if dri and n and n % dri == 0:
                if Ss:
                    sw.flush_eobrun(acc[comps[0]])
                sw.w.flush()
                sw.w.out += bytes((0xFF, 0xD0 + rst))
                rst = (rst + 1) & 7
                sw.reset()
            for c, y, x in unit:
                sw.block(c, zz[c][y][x])
        if Ss:
            sw.flush_eobrun(acc[comps[0]])
        pads.append((8 - sw.w.n) % 8)
        sw.w.flush()
        out.append(bytes(sw.w.out))
    out.append(b"\xff\xd9")
    data = b"".join(out)
    S._KNOWN[data] = q
    PAD_BITS[data] = pads
    return data


def covered(frame):
    """Per component the boolean [blocks_y, blocks_x] mask of the blocks a one-component scan covers: those that hold at least
    one sample of the component's own ceil(Xc) x ceil(Yc) size.  AC coefficients outside it are never coded."""
    hmax, vmax, mcux, mcuy = J.geometry(frame)
    out = []
    for c in frame["comps"]:
        m = np.zeros((mcuy * c["v"], mcux * c["h"]), dtype=bool)
        m[:-(-(-(-frame["H"] * c["v"] // vmax)) // 8), :-(-(-(-frame["W"] * c["h"] // hmax)) // 8)] = True
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------ the reference decoder
class _Reader:
    def __init__(self, clean):
        self.d, self.p, self.n = clean, 0, 8 * len(clean)

    def take(self, k):
        v = 0
        for _ in range(k):
            v = v << 1 | ((self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1 if self.p < self.n else 0)
            self.p += 1
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = code << 1 | self.take(1)
            s = table.get((l, code))
            if s is not None:
                return s
        raise J.JpegError("bad Huffman code")


def decode_packed(data, imgs, tabs, scans, segs):
    """Sequential decode of the packed batch, segment by segment in array order (which is file order per image) -> per image a
    list of int32 [blocks_y, blocks_x, 64] coefficient planes, natural order, as the device's coefficient buffer holds them."""
    out = [[np.zeros((im.by[c], im.bx[c], 64), dtype=np.int32) for c in range(im.ncomp)] for im in imgs]
    lookup = {}
    for sg in segs:
        sc, im = scans[sg.scan], imgs[sg.image]
        raw = bytes(data[im.data_off + sg.byte_off:im.data_off + sg.byte_off + sg.raw_len])
        br = _Reader(S.unstuff(raw))

        def table(cls, slot):
            key = (sc.tab, cls, slot)
            if key not in lookup:
                t = tabs[sc.tab]
                cnt = list(t.counts[cls * 2 + slot])
                lookup[key] = J.huff_lookup(cnt, list(t.vals[cls * 2 + slot])[:sum(cnt)])[0]
            return lookup[key]
        comps = [sc.comp[q] for q in range(sc.ncomp)]
        if sc.ncomp > 1 or sc.kind == 0:
            def unit_blocks(u):
                my, mx = divmod(u, im.mcux)
                return [(q, c, my * im.v[c] + y, mx * im.h[c] + x) for q, c in enumerate(comps) for y in range(im.v[c]) for x in range(im.h[c])]
        else:
            def unit_blocks(u):
                return [(0, comps[0], u // sc.bw, u % sc.bw)]
        blocks = [b for u in range(sg.mcu0, sg.mcu0 + sg.nmcu) for b in unit_blocks(u)]
        Ss, Se, Al = sc.ss, sc.se, sc.al
        pred = [0, 0, 0]
        eobrun = 0
        for q, c, y, x in blocks:
            blk = out[sg.image][c][y, x]
            if sc.kind in (0, 1):
                s = br.symbol(table(0, sc.td[q]))
                pred[c] += J._extend(br.take(s), s)
                blk[0] = pred[c] * (1 << Al)
            if sc.kind == 2:
                if br.take(1):
                    blk[0] |= 1 << Al
            if sc.kind in (0, 3):
                k = max(Ss, 1)
                if eobrun:
                    eobrun -= 1
                    continue
                while k <= Se:
                    rs = br.symbol(table(1, sc.ta[q]))
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        if k > Se:
                            raise J.JpegError("index past Se")
                        blk[ZZ[k]] = J._extend(br.take(s), s) * (1 << Al)
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        eobrun = (1 << r) + br.take(r) - 1
                        break
            if sc.kind == 4:
                p1 = 1 << Al

                def correct(k):
                    v = blk[ZZ[k]]
                    if br.take(1) and not (abs(v) & p1):
                        blk[ZZ[k]] = v + p1 if v > 0 else v - p1
                k = Ss
                if eobrun == 0:
                    while k <= Se:
                        rs = br.symbol(table(1, sc.ta[q]))
                        r, s = rs >> 4, rs & 15
                        if s == 0 and r < 15:
                            eobrun = (1 << r) + br.take(r)
                            break
                        if s > 1:
                            raise J.JpegError("size above 1 in a refinement scan")
                        new = (p1 if br.take(1) else -p1) if s else 0
                        while k <= Se:                         # pass r coefficients whose history is zero; stop on the next one
                            if blk[ZZ[k]]:
                                correct(k)
                            elif r == 0:
                                break
                            else:
                                r -= 1
                            k += 1
                        if s:
                            if k > Se:
                                raise J.JpegError("index past Se")
                            blk[ZZ[k]] = new
                        k += 1
                if eobrun:
                    while k <= Se:
                        if blk[ZZ[k]]:
                            correct(k)
                        k += 1
                    eobrun -= 1
        if eobrun:
            raise J.JpegError("end-of-band run past the segment's blocks")
    return out


# ------------------------------------------------------------------------------------------ the streams the tests share
SMALL_SHAPES = (("gray", 1, 1), ("gray", 8, 8), ("gray", 17, 17), ("420", 24, 40), ("420", 40, 24), ("422", 24, 40), ("422", 40, 24),
                ("420", 9, 4), ("444", 13, 21))


@functools.lru_cache(maxsize=None)
def small_source(sampling, h, w):
    return S.source(h, w, sampling, 90, seed=h * 100 + w)


@functools.lru_cache(maxsize=None)
def script_cases():
    """[(name, source, progressive stream)]: every script on every small shape, plus the table and DC-interleaving variants."""
    out = []
    for sampling, h, w in SMALL_SHAPES:
        src = small_source(sampling, h, w)
        nc = 1 if sampling == "gray" else 3
        for name, fn in SCRIPTS.items():
            out.append((f"{name} {sampling} {h}x{w}", src, recode_progressive(src, fn(nc))))
        out.append((f"dc_split {sampling} {h}x{w}", src, recode_progressive(src, pillow_script(nc), dc_interleaved=False)))
    src = small_source("420", 24, 40)
    out.append(("ids23", src, recode_progressive(src, pillow_script(3), table_ids=((2, 3, 3), (3, 2, 2)))))
    out.append(("ids_mixed", src, recode_progressive(src, approximation_script(3), table_ids=((0, 3, 3), (1, 2, 2)))))
    out.append(("one_dht", src, recode_progressive(src, pillow_script(3), one_dht=True)))
    out.append(("one_dht gray", small_source("gray", 17, 17), recode_progressive(small_source("gray", 17, 17), spectral_script(1), one_dht=True)))
    return out


@functools.lru_cache(maxsize=None)
def restart_cases():
    """[(name, source, stream)]: restart intervals 1, 2 and 7 -- MCUs in the interleaved DC scans, blocks in the AC scans --
    and Pillow's own progressive file with restart_marker_blocks=2."""
    out = []
    for sampling, h, w in (("420", 40, 24), ("422", 24, 40), ("gray", 17, 17)):
        src = small_source(sampling, h, w)
        nc = 1 if sampling == "gray" else 3
        for dri in (1, 2, 7):
            out.append((f"dri{dri} {sampling}", src, recode_progressive(src, pillow_script(nc), dri=dri)))
        out.append((f"dri2 split {sampling}", src, recode_progressive(src, approximation_script(nc), dri=2, dc_interleaved=False)))
    img = S.noisy_image(37, 70, 6)
    base = S.pillow_jpeg(img, quality=75, subsampling=2)
    out.append(("pillow restart_marker_blocks=2", base, S.pillow_jpeg(img, quality=75, subsampling=2, progressive=True, restart_marker_blocks=2)))
    return out


@functools.lru_cache(maxsize=None)
def dense_case():
    """64 x 64 at quality 95, sigma 25 noise, 4:4:4: long segments, dense history in the refinement scans."""
    src = S.source(64, 64, "444", 95, seed=11, sigma=25.0)
    return src, recode_progressive(src, pillow_script(3)), recode_progressive(src, approximation_script(3))


@functools.lru_cache(maxsize=None)
def aligned_run_case():
    """(source, stream): 32 x 32 grey, noise above, flat below, so the refinement scan ends with an end-of-band run over blocks
    without history -- and a seed at which that scan has no padding bit: the run's last blocks come behind the segment's last bit."""
    for seed in range(200):
        img = S.noisy_image(32, 32, seed)[..., 1].copy()
        img[16:] = 140
        src = S.pillow_jpeg(img, quality=90)
        data = recode_progressive(src, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)])
        if PAD_BITS[data][-1] == 0:
            return src, data
    raise AssertionError("no seed gives a refinement scan without padding bits")


def pillow_pair(arr, **kw):
    """(baseline, progressive) files Pillow writes for one image with the same quality and subsampling."""
    return S.pillow_jpeg(arr, **kw), S.pillow_jpeg(arr, progressive=True, **kw)
