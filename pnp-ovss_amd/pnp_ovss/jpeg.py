"""Host half of the device JPEG decoder (csrc/jpeg.hip, `pnp_jpeg_decode`): the reference reads every image with
`Image.open(path).convert('RGB')` (Dataset.py:349-445, PnP_OVSS_0514_updated_segmentation.py:929-955); here the host only
walks the JPEG markers (byte work: frame geometry, quantisation and Huffman tables, restart intervals) and hands the
entropy-coded bytes plus descriptors to the GPU, which does the Huffman decode, inverse DCT, chroma upsampling and colour
conversion for the whole batch.  Baseline sequential files (grayscale / YCbCr 4:4:4, 4:2:2, 4:2:0) -- what VOC / COCO /
ADE20K ship -- go through `parse` / `pack_batch`; progressive files of the same colour spaces -- what web exporters and
many phones write -- through `parse_progressive` / `pack_scans` (csrc/jpeg_prog.hip, `pnp_jpeg_decode_scans`).  Anything
else (arithmetic coding, CMYK, 12-bit, an incomplete progressive file) raises `UnsupportedJpeg` and the dataset decodes
that one file with Pillow.

Below it, the host half of the device ENCODER (csrc/jpeg_enc.hip, `pnp_jpeg_encode`): libjpeg's quality-scaled quantisation
tables and the markers around the entropy-coded scan the GPU writes, byte for byte those of Pillow's `save(..., "JPEG")`.
"""
import ctypes as C

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int32)


class UnsupportedJpeg(ValueError):
    pass


class JpegImage(C.Structure):
    _fields_ = [("data_off", C.c_int64), ("coef_off", C.c_int64 * 3), ("plane_off", C.c_int64 * 3), ("rgb_off", C.c_int64)] + \
               [(n, C.c_int32) for n in ("data_len", "H", "W", "ncomp", "hmax", "vmax", "mcux", "mcuy")] + \
               [(n, C.c_int32 * 3) for n in ("h", "v", "tq", "td", "ta", "bx", "by")] + [("tab", C.c_int32), ("pad", C.c_int32 * 2)]


class JpegTables(C.Structure):
    _fields_ = [("counts", (C.c_uint8 * 16) * 4), ("vals", (C.c_uint8 * 256) * 4), ("quant", (C.c_int32 * 64) * 4)]


class JpegSegment(C.Structure):
    _fields_ = [("byte_off", C.c_int64), ("clean_off", C.c_int64)] + \
               [(n, C.c_int32) for n in ("image", "mcu0", "nmcu", "raw_len", "clean_cap", "sub_bits", "scan", "pad")]


class JpegScan(C.Structure):
    """One scan of one image (csrc/kernels.h JpegScan).  kind: one of SCAN_KINDS.  comp / td / ta: the scan's components
    (indices into the frame) and the slot (0 / 1) of each one's DC / AC table in the JpegTables entry `tab`, the snapshot of
    the Huffman tables in force at this SOS.  bw x bh: the grid the scan's units are counted on -- MCUs of the frame for an
    interleaved scan, the component's own ceil(Xc / 8) x ceil(Yc / 8) blocks for a one-component scan."""
    _fields_ = [(n, C.c_int32) for n in ("image", "kind", "ordinal", "ncomp")] + [(n, C.c_int32 * 3) for n in ("comp", "td", "ta")] + \
               [(n, C.c_int32) for n in ("ss", "se", "ah", "al", "tab", "bw", "bh", "nunits")] + [("pad", C.c_int32 * 3)]


SCAN_KINDS = ("sequential", "dc_first", "dc_refine", "ac_first", "ac_refine")
MAX_SCANS = 64          # scans per progressive file; a file with more goes to Pillow

SUBSEQUENCES = 1024     # threads per restart segment of the device decoder (csrc/jpeg.hip JPEG_T)


def _u16(b, p):
    return (b[p] << 8) | b[p + 1]


def parse(data: bytes):
    """Marker walk of one file -> dict(H, W, comps[{h, v, tq, td, ta}], qt{id: int32[64] natural order},
    ht{(class, id): (counts[16], symbols)}, dri, scan_start, scan_end).  Anything the device decoder does not cover --
    including truncated / malformed marker segments and 3-component files that are NOT YCbCr (Adobe APP14 transform 0,
    or component ids 'R','G','B': libjpeg would not colour-convert them) -- raises UnsupportedJpeg, so the caller falls
    back to Pillow instead of failing or silently converting the wrong colour space."""
    try:
        return _parse(data)
    except UnsupportedJpeg:
        raise
    except (IndexError, ValueError, KeyError) as exc:
        raise UnsupportedJpeg(f"malformed marker segment ({type(exc).__name__}: {exc})") from None


def _parse(data: bytes):
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG stream")
    pos, n = 2, len(data)
    qt, ht, comps, H, W, dri = {}, {}, None, 0, 0, 0
    adobe_transform = None
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            raise UnsupportedJpeg("marker expected")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0xD9:
            break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        L = _u16(data, pos)
        seg = data[pos + 2:pos + L]
        if m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                p += 1
                if pq:
                    vals = [_u16(seg, p + 2 * i) for i in range(64)]
                    p += 128
                else:
                    vals = list(seg[p:p + 64])
                    p += 64
                t = np.zeros(64, dtype=np.int32)
                t[ZIGZAG] = vals
                qt[tq] = t
        elif m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise UnsupportedJpeg("sample precision is not 8 bits")
            H, W, nc = _u16(seg, 1), _u16(seg, 3), seg[5]
            comps = [dict(id=seg[6 + 3 * i], h=seg[7 + 3 * i] >> 4, v=seg[7 + 3 * i] & 15, tq=seg[8 + 3 * i]) for i in range(nc)]
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise UnsupportedJpeg(f"SOF{m - 0xC0}: progressive / lossless / arithmetic coding")
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                counts = list(seg[p + 1:p + 17])
                ns = sum(counts)
                ht[(tc, th)] = (counts, list(seg[p + 17:p + 17 + ns]))
                p += 17 + ns
        elif m == 0xDD:
            dri = _u16(seg, 0)
        elif m == 0xEE and len(seg) >= 12 and bytes(seg[:5]) == b"Adobe":
            adobe_transform = seg[11]                  # 0: no colour transform (RGB / CMYK), 1: YCbCr, 2: YCCK
        elif m == 0xDA:
            if comps is None:
                raise UnsupportedJpeg("scan before frame header")
            ns = seg[0]
            if ns != len(comps):
                raise UnsupportedJpeg("non-interleaved scans")
            for i in range(ns):
                c = [c for c in comps if c["id"] == seg[1 + 2 * i]][0]
                c["td"], c["ta"] = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
            start = pos + L
            end = data.rfind(b"\xff\xd9")
            if end < start:
                end = n
            if len(comps) == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            elif len(comps) == 3:
                if adobe_transform == 0 or [c["id"] for c in comps] == [82, 71, 66]:
                    raise UnsupportedJpeg("3-component file stored as RGB, not YCbCr (Adobe transform 0 / component ids R,G,B)")
                c0 = comps[0]
                if not (comps[1]["h"] == comps[2]["h"] == comps[1]["v"] == comps[2]["v"] == 1 and
                        (c0["h"], c0["v"]) in ((1, 1), (2, 1), (2, 2))):
                    raise UnsupportedJpeg("chroma sampling other than 4:4:4 / 4:2:2 / 4:2:0")
            else:
                raise UnsupportedJpeg(f"{len(comps)} components")
            for c in comps:
                if c["tq"] not in qt or (0, c["td"]) not in ht or (1, c["ta"]) not in ht or c["td"] > 1 or c["ta"] > 1 or c["tq"] > 3:
                    raise UnsupportedJpeg("missing table")
            return dict(H=H, W=W, comps=comps, qt=qt, ht=ht, dri=dri, scan_start=start, scan_end=end)
        pos += L
    raise UnsupportedJpeg("no scan")


def _fill_tables(tab, j):
    """The file's DHT (code counts per length, symbols) and DQT tables as they are; the device builds its look-ahead tables
    (T.81 F.2.2.3 canonical codes) from them."""
    for (tc, th), (counts, symbols) in j["ht"].items():
        if th > 1:
            continue
        if sum(counts) > 256 or len(symbols) != sum(counts):
            raise UnsupportedJpeg("bad Huffman table")
        t = tc * 2 + th
        tab.counts[t][:] = counts
        tab.vals[t][:len(symbols)] = symbols
    for tq, q in j["qt"].items():
        if tq < 4:
            tab.quant[tq][:] = q.tolist()


def _table_key(j):
    return (tuple(sorted((k, tuple(c), tuple(v)) for k, (c, v) in j["ht"].items())), tuple(sorted((k, q.tobytes()) for k, q in j["qt"].items())))


def pack_batch(files):
    """list of JPEG byte strings -> (data uint8 array, JpegImage[], JpegTables[], JpegSegment[], sizes, totals) ready to
    upload.  totals = dict(coef_elems, plane_bytes, rgb_bytes, clean_bytes, max_blocks, max_pixels).  Files with the same
    DHT + DQT bytes (every file an encoder wrote with its default tables at one quality) share one JpegTables entry."""
    n = len(files)
    imgs = (JpegImage * n)()
    tab_index, tab_list = {}, []
    segs = []
    chunks, data_off = [], 0
    coef = plane = rgb = clean = 0
    max_blocks = max_pixels = 0
    sizes = []
    for i, f in enumerate(files):
        j = parse(f)
        comps = j["comps"]
        hmax = max(c["h"] for c in comps)
        vmax = max(c["v"] for c in comps)
        mcux = -(-j["W"] // (8 * hmax))
        mcuy = -(-j["H"] // (8 * vmax))
        scan = np.frombuffer(f, dtype=np.uint8, count=j["scan_end"] - j["scan_start"], offset=j["scan_start"])
        im = imgs[i]
        im.data_off, im.data_len = data_off, len(scan)
        im.H, im.W, im.ncomp, im.hmax, im.vmax, im.mcux, im.mcuy = j["H"], j["W"], len(comps), hmax, vmax, mcux, mcuy
        blocks = 0
        for ci, c in enumerate(comps):
            im.h[ci], im.v[ci], im.tq[ci], im.td[ci], im.ta[ci] = c["h"], c["v"], c["tq"], c["td"], c["ta"]
            im.bx[ci], im.by[ci] = mcux * c["h"], mcuy * c["v"]
            nb = im.bx[ci] * im.by[ci]
            im.coef_off[ci], im.plane_off[ci] = coef, plane
            coef += nb * 64
            plane += nb * 64
            blocks += nb
        im.rgb_off = rgb
        key = _table_key(j)
        if key not in tab_index:
            tab_index[key] = len(tab_list)
            t = JpegTables()
            _fill_tables(t, j)
            tab_list.append(t)
        im.tab = tab_index[key]
        rgb += j["H"] * j["W"] * 3
        sizes.append((j["H"], j["W"]))
        max_blocks = max(max_blocks, blocks)
        max_pixels = max(max_pixels, j["H"] * j["W"])
        # restart intervals: every RSTn marker starts an independently decodable segment
        nmcu = mcux * mcuy
        starts, ends = [0], []
        if j["dri"]:
            ff = np.flatnonzero(scan[:-1] == 0xFF)
            rst = ff[(scan[ff + 1] >= 0xD0) & (scan[ff + 1] <= 0xD7)]
            starts += [int(p) + 2 for p in rst]
            ends = [int(p) for p in rst]
        ends.append(len(scan))
        for k, (s0, s1) in enumerate(zip(starts, ends)):
            m0 = k * j["dri"] if j["dri"] else 0
            if m0 >= nmcu:
                break
            raw = s1 - s0
            cap = ((raw + 15) & ~15) + 32
            sub = max(128, (-(-raw * 8 // SUBSEQUENCES) + 31) & ~31)
            segs.append((s0, clean, i, m0, min(j["dri"], nmcu - m0) if j["dri"] else nmcu, raw, cap, sub))
            clean += cap
        chunks.append(scan)
        pad = (-len(scan)) % 16
        if pad:
            chunks.append(np.zeros(pad, dtype=np.uint8))
        data_off += len(scan) + pad
    tabs = (JpegTables * len(tab_list))(*tab_list)
    sg = (JpegSegment * len(segs))()
    for k, (off, coff, i, m0, nm, raw, cap, sub) in enumerate(segs):
        g = sg[k]
        g.byte_off, g.clean_off, g.image, g.mcu0, g.nmcu, g.raw_len, g.clean_cap, g.sub_bits = off, coff, i, m0, nm, raw, cap, sub
    data = np.concatenate(chunks) if chunks else np.zeros(16, dtype=np.uint8)
    return data, imgs, tabs, sg, sizes, dict(coef_elems=coef, plane_bytes=plane, rgb_bytes=rgb, clean_bytes=clean, max_blocks=max_blocks,
                                             max_pixels=max_pixels)


# ---------------------------------------------------------------------------------------------------------- progressive files
# SOF2 (csrc/jpeg_prog.hip, `pnp_jpeg_decode_scans`): the coefficients arrive in several scans (T.81 Annex G), each a band
# Ss..Se of the zig-zag sequence of some components at some bit precision.  The host records every scan and checks the
# progression (T.81 G.1.1.1.1); the device decodes them in file order into the same coefficient buffers as a baseline file.
def parse_progressive(data: bytes):
    """Marker walk of one SOF2 file (8-bit, Huffman, greyscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0) -> dict(H, W, comps[{id, h,
    v, tq, q}], scans[{comps, td, ta, Ss, Se, Ah, Al, kind, start, end, dri, ht}]): per scan the component indices, the
    table SLOTS (0 / 1) of each component, the entropy-coded byte range, the restart interval and the snapshot
    {(class, slot): (counts, symbols)} of the Huffman tables in force at that SOS.  comps[c]['q'] is the quantisation table
    in force at the component's first scan.  Raises UnsupportedJpeg for what the device does not decode: other processes and
    colour spaces (as `parse`), a scan that breaks the progression rules, an incomplete file (some coefficient never reaches
    Al = 0: libjpeg would smooth it), more than MAX_SCANS scans, more than two tables of one class in one scan."""
    try:
        return _parse_progressive(data)
    except UnsupportedJpeg:
        raise
    except (IndexError, ValueError, KeyError) as exc:
        raise UnsupportedJpeg(f"malformed marker segment ({type(exc).__name__}: {exc})") from None


def _scan_end(marks, start, n):
    """First byte behind the entropy-coded data that starts at `start`: the next FF that neither a stuffed 00 nor RSTn follows."""
    k = int(np.searchsorted(marks, start))
    return int(marks[k]) if k < len(marks) else n


def _parse_progressive(data: bytes):
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG stream")
    a = np.frombuffer(data, dtype=np.uint8)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nx = a[ff + 1]
    marks = ff[(nx != 0) & ~((nx >= 0xD0) & (nx <= 0xD7))]
    pos, n = 2, len(data)
    qt, ht, comps, H, W, dri = {}, {}, None, 0, 0, 0
    adobe_transform = None
    scans, al = [], None                              # al[c][k]: the point transform coefficient k of component c stands at, -1 = not seen
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            raise UnsupportedJpeg("marker expected")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0xD9:
            break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        L = _u16(data, pos)
        seg = data[pos + 2:pos + L]
        if m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                p += 1
                if pq:
                    vals = [_u16(seg, p + 2 * i) for i in range(64)]
                    p += 128
                else:
                    vals = list(seg[p:p + 64])
                    p += 64
                t = np.zeros(64, dtype=np.int32)
                t[ZIGZAG] = vals
                qt[tq] = t
        elif m == 0xC2:
            if comps is not None:
                raise UnsupportedJpeg("second frame header")
            if seg[0] != 8:
                raise UnsupportedJpeg("sample precision is not 8 bits")
            H, W, nc = _u16(seg, 1), _u16(seg, 3), seg[5]
            comps = [dict(id=seg[6 + 3 * i], h=seg[7 + 3 * i] >> 4, v=seg[7 + 3 * i] & 15, tq=seg[8 + 3 * i]) for i in range(nc)]
            if H == 0 or W == 0:
                raise UnsupportedJpeg("frame without a size (DNL)")
            if nc == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            elif nc == 3:
                c0 = comps[0]
                if not (comps[1]["h"] == comps[2]["h"] == comps[1]["v"] == comps[2]["v"] == 1 and
                        (c0["h"], c0["v"]) in ((1, 1), (2, 1), (2, 2))):
                    raise UnsupportedJpeg("chroma sampling other than 4:4:4 / 4:2:2 / 4:2:0")
            else:
                raise UnsupportedJpeg(f"{nc} components")
            al = [[-1] * 64 for _ in comps]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise UnsupportedJpeg(f"SOF{m - 0xC0}: not a progressive Huffman file")
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                counts = list(seg[p + 1:p + 17])
                ns = sum(counts)
                if tc > 1 or th > 3 or ns > 256 or p + 17 + ns > len(seg):
                    raise UnsupportedJpeg("bad Huffman table")
                ht[(tc, th)] = (counts, list(seg[p + 17:p + 17 + ns]))
                p += 17 + ns
        elif m == 0xDD:
            dri = _u16(seg, 0)
        elif m == 0xEE and len(seg) >= 12 and bytes(seg[:5]) == b"Adobe":
            adobe_transform = seg[11]
        elif m == 0xDA:
            if comps is None:
                raise UnsupportedJpeg("scan before frame header")
            if len(comps) == 3 and (adobe_transform == 0 or [c["id"] for c in comps] == [82, 71, 66]):
                raise UnsupportedJpeg("3-component file stored as RGB, not YCbCr (Adobe transform 0 / component ids R,G,B)")
            if len(scans) >= MAX_SCANS:
                raise UnsupportedJpeg(f"more than {MAX_SCANS} scans")
            ns = seg[0]
            if not 1 <= ns <= len(comps) or len(seg) != 4 + 2 * ns:
                raise UnsupportedJpeg("bad scan header")
            ids = [c["id"] for c in comps]
            sc = [ids.index(seg[1 + 2 * i]) for i in range(ns)]
            if sorted(set(sc)) != sc:
                raise UnsupportedJpeg("scan components out of frame order")
            if ns == 2:
                raise UnsupportedJpeg("scan of two components")       # (legal, but no encoder writes it: its MCU is not the frame's)
            td = [seg[2 + 2 * i] >> 4 for i in range(ns)]
            ta = [seg[2 + 2 * i] & 15 for i in range(ns)]
            Ss, Se, Ah, Al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            if Ss == 0:
                if Se != 0:
                    raise UnsupportedJpeg("DC and AC coefficients in one progressive scan")
            elif ns != 1:
                raise UnsupportedJpeg("AC scan of more than one component")
            elif not Ss <= Se <= 63:
                raise UnsupportedJpeg("bad spectral selection")
            if Al > 13 or (Ah and Al != Ah - 1):
                raise UnsupportedJpeg("bad successive approximation")
            for c in sc:
                if Ss and al[c][0] < 0:
                    raise UnsupportedJpeg("AC scan before the component's first DC scan")
                for k in range(Ss, Se + 1):
                    if (Ah == 0 and al[c][k] >= 0) or (Ah and al[c][k] != Ah):
                        raise UnsupportedJpeg(f"coefficient {k} of component {c}: Ah = {Ah} where the previous Al is {al[c][k]}")
                    al[c][k] = Al
                if "q" not in comps[c]:
                    if comps[c]["tq"] not in qt:
                        raise UnsupportedJpeg("missing table")
                    comps[c]["q"] = qt[comps[c]["tq"]].copy()
            kind = (1 if Ah == 0 else 2) if Ss == 0 else (3 if Ah == 0 else 4)
            used = [] if kind == 2 else (sorted(set(td)) if kind == 1 else sorted(set(ta)))
            tc = 0 if kind == 1 else 1
            if len(used) > 2:
                raise UnsupportedJpeg("more than two Huffman tables of one class in one scan")
            snap = {}
            for slot, th in enumerate(used):
                if th > 3 or (tc, th) not in ht:
                    raise UnsupportedJpeg("missing table")
                snap[(tc, slot)] = ht[(tc, th)]
            start = pos + L
            end = _scan_end(marks, start, n)
            scans.append(dict(comps=sc, td=[used.index(t) if kind == 1 else 0 for t in td],
                              ta=[used.index(t) if kind >= 3 else 0 for t in ta], Ss=Ss, Se=Se, Ah=Ah, Al=Al, kind=kind, start=start,
                              end=end, dri=dri, ht=snap))
            pos = end
            continue
        pos += L
    if comps is None or not scans:
        raise UnsupportedJpeg("no scan")
    if any(x != 0 for row in al for x in row):
        raise UnsupportedJpeg("incomplete progressive file: some coefficient never reaches Al = 0")
    return dict(H=H, W=W, comps=comps, scans=scans)


def _scan_tables(ht, qtabs):
    """A JpegTables entry from {(class, slot): (counts, symbols)} and {tq: table}; its key for sharing by content."""
    t = JpegTables()
    for (tc, slot), (counts, symbols) in ht.items():
        if sum(counts) > 256 or len(symbols) != sum(counts):
            raise UnsupportedJpeg("bad Huffman table")
        t.counts[tc * 2 + slot][:] = counts
        t.vals[tc * 2 + slot][:len(symbols)] = symbols
    for tq, q in qtabs.items():
        t.quant[tq][:] = q.tolist()
    key = (tuple(sorted((k, tuple(c), tuple(v)) for k, (c, v) in ht.items())), tuple(sorted((k, q.tobytes()) for k, q in qtabs.items())))
    return t, key


def _restart_segments(scan, dri, nunits):
    """[(first byte, bytes, first unit, units)] of the restart intervals of one scan's entropy-coded bytes."""
    starts, ends = [0], []
    if dri:
        ff = np.flatnonzero(scan[:-1] == 0xFF)
        rst = ff[(scan[ff + 1] >= 0xD0) & (scan[ff + 1] <= 0xD7)]
        starts += [int(p) + 2 for p in rst]
        ends = [int(p) for p in rst]
    ends.append(len(scan))
    out = []
    for k, (s0, s1) in enumerate(zip(starts, ends)):
        u0 = k * dri if dri else 0
        if u0 >= nunits:
            break
        out.append((s0, s1 - s0, u0, min(dri, nunits - u0) if dri else nunits))
    return out


def is_progressive(data: bytes):
    """True where `parse_progressive`, not `parse`, is the parser to try: the first SOFn marker of the file is SOF2."""
    pos, n = 2, len(data)
    while pos + 4 <= n and data[pos] == 0xFF:
        while pos < n and data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m == 0xC2
        if m in (0xD9, 0xDA):
            return False
        if not (m == 0x01 or 0xD0 <= m <= 0xD7):
            pos += _u16(data, pos)
    return False


def pack_scans(files):
    """Any mix of baseline and progressive files -> (data, JpegImage[], JpegTables[], JpegScan[], JpegSegment[], groups, sizes,
    totals) for `pnp_jpeg_decode_scans`.  Images, coefficient / plane / RGB offsets and totals as `pack_batch`.  A baseline
    file is one scan of kind 'sequential'; a progressive file has one JpegScan per SOS, each with the JpegTables entry of its
    own Huffman snapshot (the image's own entry holds the quantisation tables).  One restart interval of one scan is one
    segment; its mcu0 / nmcu count the scan's units (MCUs, or blocks of a one-component scan).  Segments are ordered baseline
    first, then by (scan ordinal, kind, image): `groups` is an int32 array [n, 4] of (first segment, segments, kind, ordinal),
    one kernel launch each, and totals['base_segments'] the number of baseline segments in front."""
    n = len(files)
    imgs = (JpegImage * n)()
    tab_index, tab_list = {}, []
    scans, segs = [], []                              # segs: (ordinal, kind, image, scan index, byte_off, raw, unit0, units)
    chunks, data_off = [], 0
    coef = plane = rgb = 0
    max_blocks = max_pixels = 0
    sizes = []

    def table(ht, qtabs):
        t, key = _scan_tables(ht, qtabs)
        if key not in tab_index:
            tab_index[key] = len(tab_list)
            tab_list.append(t)
        return tab_index[key]

    for i, f in enumerate(files):
        prog = is_progressive(f)
        j = parse_progressive(f) if prog else parse(f)
        comps = j["comps"]
        hmax = max(c["h"] for c in comps)
        vmax = max(c["v"] for c in comps)
        mcux = -(-j["W"] // (8 * hmax))
        mcuy = -(-j["H"] // (8 * vmax))
        lo, hi = (j["scans"][0]["start"], max(s["end"] for s in j["scans"])) if prog else (j["scan_start"], j["scan_end"])
        raw = np.frombuffer(f, dtype=np.uint8, count=hi - lo, offset=lo)
        im = imgs[i]
        im.data_off, im.data_len = data_off, len(raw)
        im.H, im.W, im.ncomp, im.hmax, im.vmax, im.mcux, im.mcuy = j["H"], j["W"], len(comps), hmax, vmax, mcux, mcuy
        blocks = 0
        for ci, c in enumerate(comps):
            im.h[ci], im.v[ci], im.tq[ci] = c["h"], c["v"], (ci if prog else c["tq"])
            im.td[ci], im.ta[ci] = (0, 0) if prog else (c["td"], c["ta"])
            im.bx[ci], im.by[ci] = mcux * c["h"], mcuy * c["v"]
            nb = im.bx[ci] * im.by[ci]
            im.coef_off[ci], im.plane_off[ci] = coef, plane
            coef += nb * 64
            plane += nb * 64
            blocks += nb
        im.rgb_off = rgb
        rgb += j["H"] * j["W"] * 3
        sizes.append((j["H"], j["W"]))
        max_blocks = max(max_blocks, blocks)
        max_pixels = max(max_pixels, j["H"] * j["W"])
        if prog:
            im.tab = table({}, {ci: c["q"] for ci, c in enumerate(comps)})       # (quantisation latched per component: slot = component)
            file_scans = j["scans"]
        else:
            key = _table_key(j)
            if ("base", key) not in tab_index:
                tab_index[("base", key)] = len(tab_list)
                t = JpegTables()
                _fill_tables(t, j)
                tab_list.append(t)
            im.tab = tab_index[("base", key)]
            file_scans = [dict(comps=list(range(len(comps))), td=[c["td"] for c in comps], ta=[c["ta"] for c in comps], Ss=0, Se=63,
                               Ah=0, Al=0, kind=0, start=lo, end=hi, dri=j["dri"], ht=None)]
        for o, s in enumerate(file_scans):
            sc = JpegScan()
            sc.image, sc.kind, sc.ordinal, sc.ncomp = i, s["kind"], o, len(s["comps"])
            for q, ci in enumerate(s["comps"]):
                sc.comp[q], sc.td[q], sc.ta[q] = ci, s["td"][q], s["ta"][q]
            sc.ss, sc.se, sc.ah, sc.al = s["Ss"], s["Se"], s["Ah"], s["Al"]
            sc.tab = im.tab if s["ht"] is None else table(s["ht"], {})
            if len(s["comps"]) == 1 and s["kind"]:
                c = comps[s["comps"][0]]
                sc.bw = -(-(-(-j["W"] * c["h"] // hmax)) // 8)
                sc.bh = -(-(-(-j["H"] * c["v"] // vmax)) // 8)
            else:
                sc.bw, sc.bh = mcux, mcuy
            sc.nunits = sc.bw * sc.bh
            body = raw[s["start"] - lo:s["end"] - lo]
            for s0, ln, u0, nu in _restart_segments(body, s["dri"], sc.nunits):
                segs.append((o if s["kind"] else -1, s["kind"], i, len(scans), s["start"] - lo + s0, ln, u0, nu))
            scans.append(sc)
        chunks.append(raw)
        pad = (-len(raw)) % 16
        if pad:
            chunks.append(np.zeros(pad, dtype=np.uint8))
        data_off += len(raw) + pad
    segs.sort(key=lambda g: g[:3])                    # (stable: the restart intervals of a scan stay in order)
    sg = (JpegSegment * len(segs))()
    groups, clean = [], 0
    for k, (o, kind, i, si, off, ln, u0, nu) in enumerate(segs):
        g = sg[k]
        cap = ((ln + 15) & ~15) + 32
        g.byte_off, g.clean_off, g.image, g.mcu0, g.nmcu, g.raw_len, g.clean_cap, g.scan = off, clean, i, u0, nu, ln, cap, si
        g.sub_bits = max(128, (-(-ln * 8 // SUBSEQUENCES) + 31) & ~31)
        clean += cap
        if kind:
            if groups and groups[-1][2:] == [kind, o]:
                groups[-1][1] += 1
            else:
                groups.append([k, 1, kind, o])
    tabs = (JpegTables * len(tab_list))(*tab_list)
    sc_arr = (JpegScan * len(scans))(*scans)
    data = np.concatenate(chunks) if chunks else np.zeros(16, dtype=np.uint8)
    totals = dict(coef_elems=coef, plane_bytes=plane, rgb_bytes=rgb, clean_bytes=clean, max_blocks=max_blocks, max_pixels=max_pixels,
                  base_segments=sum(1 for g in segs if g[1] == 0))
    return data, imgs, tabs, sc_arr, sg, np.asarray(groups, dtype=np.int32).reshape(-1, 4), sizes, totals


# ---------------------------------------------------------------------------------------------------------- encoder, host half
# The device (csrc/jpeg_enc.hip, `pnp_jpeg_encode`) produces the entropy-coded scan; the markers around it are written here,
# byte for byte what libjpeg writes for Pillow's `Image.save(buf, "JPEG", quality=q)`: SOI, APP0 (JFIF 1.01, aspect 1:1),
# two DQT segments, SOF0 (Y 2x2, Cb / Cr 1x1), four DHT segments (T.81 Annex K.3: DC0, AC0, DC1, AC1), SOS -- scan -- EOI.
STD_LUMA_QUANT = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22,
                           29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87,
                           103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
STD_CHROMA_QUANT = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                             47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)
STD_DHT = (
    (0x00, bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0x10, bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0x11, bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
)


def quality_tables(quality=75):
    """libjpeg's jpeg_set_quality (force_baseline): uint16 [2, 64], luma and chroma, natural order."""
    q = int(quality)
    if not 1 <= q <= 95:
        raise ValueError(f"quality {quality!r}: 1..95 (Pillow's range for the standard tables)")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * s + 50) // 100, 1, 255) for b in (STD_LUMA_QUANT, STD_CHROMA_QUANT)]).astype(np.uint16)


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def encode_headers(H, W, quant):
    """Everything in front of the entropy-coded scan, for an H x W image and the tables of quality_tables()."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG frames are 1..65535 pixels a side, not {H} x {W}")
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for t in (0, 1):
        out.append(_segment(0xDB, bytes((t,)) + bytes(int(v) for v in np.asarray(quant[t])[ZIGZAG])))
    out.append(_segment(0xC0, bytes((8,)) + int(H).to_bytes(2, "big") + int(W).to_bytes(2, "big") +
                        bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))))
    for tc_th, counts, symbols in STD_DHT:
        out.append(_segment(0xC4, bytes((tc_th,)) + counts + symbols))
    out.append(_segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(out)


def scan_capacity(H, W, worst=False):
    """Bytes to reserve for an image's scan.  Default: 1.5 bytes per pixel of the MCU grid (the size of the raw 4:2:0 samples;
    photographs and overlays need a fraction of it).  worst=True: the bound no input exceeds -- every block at its longest
    codes (20 + 63 * 26 bits) and every byte stuffed."""
    mcus = -(-H // 16) * -(-W // 16)
    return mcus * 6 * 416 + 16 if worst else mcus * 384 + 64
