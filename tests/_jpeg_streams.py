"""A baseline JPEG stream writer for the decoder tests (test_jpeg_streams_cpu.py, test_jpeg_ops_gpu.py): plain Python and numpy,
independent of the code under test except for the oracle's parser (oracle/jpeg_np.py).

`recode` takes a stream Pillow encoded, recovers its QUANTISED coefficients (the oracle's entropy decode divided by the
quantisation table; the division is asserted exact) and codes them again with parameters no Pillow encoder chooses: arbitrary
Huffman tables, any table id per component, restart intervals, one DHT segment for all tables, 16-bit DQT under SOF1, other
component ids, fill bytes, COM / APPn / Adobe segments, no JFIF, bytes behind EOI.  The coefficients are never synthesised:
they come from libjpeg's forward DCT of 8-bit pixels, so every libjpeg IDCT path (SIMD or C) clamps them the same way and the
expected pixels -- Pillow's own decode of the re-coded stream -- are defined.

Table sets (all legal: Kraft sum below 1, no all-ones code), each a (DC, AC) pair of (counts[16], symbols):
  unary   DC: one symbol at each length 1..12 (two codes longer than a 10-bit look-ahead); AC: T.81 K.3 luminance
  skewed  DC: T.81 K.3 luminance; AC: one symbol at each length 1..8, the other 154 standard symbols at length 16 (the long-code
          path all the time, dense FF bytes and stuffing)
  flat    DC: 12 symbols at length 4; AC: 162 symbols at length 8 (fixed-length codes do not self-synchronise, and the codes
          162..255 / 12..15 stay undefined)
"""
import functools
import io

import numpy as np
from PIL import Image

from oracle import jpeg_np as J

ZZ = J.ZIGZAG

STD_DC = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_AC = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
_AC_SHORT = [0x00, 0x01, 0x02, 0x11, 0x03, 0x21, 0x12, 0x04]
UNARY_DC = ([1] * 12 + [0] * 4, list(range(12)))
SKEWED_AC = ([1] * 8 + [0] * 7 + [154], _AC_SHORT + [s for s in STD_AC[1] if s not in _AC_SHORT])
FLAT_DC = ([0] * 3 + [12] + [0] * 12, list(range(12)))
FLAT_AC = ([0] * 7 + [162] + [0] * 8, list(STD_AC[1]))

TABLE_SETS = {"unary": (UNARY_DC, STD_AC), "skewed": (STD_DC, SKEWED_AC), "flat": (FLAT_DC, FLAT_AC)}
_OTHER = {"unary": "skewed", "skewed": "flat", "flat": "unary"}         # the set on the table id the luma does not use
ASSIGNMENTS = ("shared0", "luma1", "one_dht")
SAMPLINGS = ("444", "422", "420", "gray")


def check_tables_legal(counts, symbols):
    """Kraft sum below 1 (so no code is all ones), as many symbols as codes, no symbol twice."""
    assert len(counts) == 16 and sum(counts) == len(symbols) == len(set(symbols))
    assert sum(c << (16 - l) for l, c in enumerate(counts, 1)) < 1 << 16


def assignment(name, nc, tset):
    """-> (tables {(class, id): (counts, symbols)}, [(td, ta)] per component, one_dht) for one of ASSIGNMENTS:
    shared0: every component on table 0, only that pair in the file; luma1: luma on table 1, chroma on table 0, which holds
    another set; one_dht: luma 0 / chroma 1, all four tables in one DHT segment."""
    dc, ac = TABLE_SETS[tset]
    odc, oac = TABLE_SETS[_OTHER[tset]]
    if name == "shared0":
        return {(0, 0): dc, (1, 0): ac}, [(0, 0)] * nc, False
    if name == "luma1":
        return {(0, 0): odc, (1, 0): oac, (0, 1): dc, (1, 1): ac}, [(1, 1)] + [(0, 0)] * (nc - 1), False
    if name == "one_dht":
        return {(0, 0): dc, (1, 0): ac, (0, 1): odc, (1, 1): oac}, [(0, 0)] + [(1, 1)] * (nc - 1), True
    raise KeyError(name)


# ------------------------------------------------------------------------------------------ images and Pillow
def noisy_image(h, w, seed, sigma=25.0):
    """Smooth colour waves plus Gaussian noise: every coefficient position is populated at high quality."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / 7. + yy / 9.), 128 + 80 * np.cos(xx / 5. - yy / 3.), (xx * 3 + 2 * yy) % 256], -1)
    return np.clip(base + rng.normal(0, sigma, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_jpeg(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def source(h, w, sampling, quality, seed=0, sigma=25.0, **kw):
    """A Pillow-encoded stream of noisy_image(h, w, seed): sampling one of SAMPLINGS."""
    img = noisy_image(h, w, seed, sigma)
    if sampling == "gray":
        return pillow_jpeg(img[..., 1], quality=quality, **kw)
    return pillow_jpeg(img, quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)


# ------------------------------------------------------------------------------------------ coefficients of a stream
_KNOWN = {}           # stream bytes -> quantised coefficients, for streams this module wrote (spares the slow oracle decode)


def quantised(data):
    """-> (parsed stream, [int32 [blocks_y, blocks_x, 64] per component]): the quantised coefficients in natural order."""
    j = J.parse_jpeg(data)
    J.geometry(j["frame"])
    if data in _KNOWN:
        return j, _KNOWN[data]
    deq = J.decode_coefficients(j)
    out = []
    for c, d in zip(j["frame"]["comps"], deq):
        qt = j["qt"][c["tq"]]
        q = d // qt
        assert np.array_equal(q * qt, d), "dequantised coefficients are not multiples of the quantisation table"
        out.append(q)
    _KNOWN[data] = out
    return j, out


# ------------------------------------------------------------------------------------------ the writer
def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def _codes(counts, symbols):
    return {s: (c, l) for (l, c), s in J.huff_lookup(counts, symbols)[0].items()}


class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(w, v, s):
    if s:
        w.put(v if v > 0 else v + (1 << s) - 1, s)


ADOBE = {t: _segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes((t,))) for t in (0, 1, 2)}
JFIF = _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def recode(src, tables=None, use=None, dri=0, one_dht=False, dqt16=False, ids=None, gray_factors=None, jfif=True, adobe=None,
           fill=0, com=None, app=None, trailing=b""):
    """Re-code the Pillow stream `src`.
    tables {(class, id): (counts, symbols)} and use [(td, ta)] per component (default: the source's own); dri: restart
    interval in MCUs; one_dht: all tables in one DHT segment; dqt16: 16-bit DQT (Pq = 1) under SOF1; ids: component ids;
    gray_factors (h, v): sampling factors written into the SOF of a one-component file; jfif: APP0 present; adobe: transform
    of an APP14 segment; fill: number of FF fill bytes in front of every marker behind SOI; com / app: payload of a COM /
    APP5 segment; trailing: bytes behind EOI."""
    j, q = quantised(src)
    frame = j["frame"]
    comps = frame["comps"]
    _, _, mcux, mcuy = J.geometry(frame)
    tables = dict(j["ht"]) if tables is None else tables
    use = [(c["td"], c["ta"]) for c in comps] if use is None else use
    ids = [c["id"] for c in comps] if ids is None else ids
    for t in tables.values():
        check_tables_legal(*t)
    cm = {k: _codes(*v) for k, v in tables.items()}
    w, pred, n, rst = _BitWriter(), [0] * len(comps), 0, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if dri and n and n % dri == 0:
                w.flush()
                w.out += bytes((0xFF, 0xD0 + rst))
                rst = (rst + 1) & 7
                pred = [0] * len(comps)
            n += 1
            for ci, c in enumerate(comps):
                dc, ac = cm[(0, use[ci][0])], cm[(1, use[ci][1])]
                for by in range(c["v"]):
                    for bx in range(c["h"]):
                        z = [int(v) for v in q[ci][my * c["v"] + by, mx * c["h"] + bx][ZZ]]
                        d = z[0] - pred[ci]
                        pred[ci] = z[0]
                        s = abs(d).bit_length()
                        w.put(*dc[s])
                        _magnitude(w, d, s)
                        run, last = 0, max([k for k in range(1, 64) if z[k]] or [0])
                        for k in range(1, last + 1):
                            v = z[k]
                            if v == 0:
                                run += 1
                                continue
                            while run > 15:
                                w.put(*ac[0xF0])
                                run -= 16
                            s = abs(v).bit_length()
                            w.put(*ac[(run << 4) | s])
                            _magnitude(w, v, s)
                            run = 0
                        if last < 63:
                            w.put(*ac[0])
    w.flush()
    head = []
    if jfif:
        head.append(JFIF)
    if adobe is not None:
        head.append(ADOBE[adobe])
    if app is not None:
        head.append(_segment(0xE5, app))
    if com is not None:
        head.append(_segment(0xFE, com))
    for t, qq in j["qt"].items():
        zz = [int(x) for x in qq[ZZ]]
        head.append(_segment(0xDB, bytes((0x10 | t,)) + b"".join(x.to_bytes(2, "big") for x in zz)) if dqt16
                    else _segment(0xDB, bytes((t,)) + bytes(zz)))
    sof = bytes((8,)) + frame["H"].to_bytes(2, "big") + frame["W"].to_bytes(2, "big") + bytes((len(comps),))
    for ci, c in enumerate(comps):
        h, v = gray_factors if (gray_factors and len(comps) == 1) else (c["h"], c["v"])
        sof += bytes((ids[ci], h << 4 | v, c["tq"]))
    head.append(_segment(0xC1 if dqt16 else 0xC0, sof))
    dht = [bytes((tc << 4 | th,)) + bytes(cnt) + bytes(sym) for (tc, th), (cnt, sym) in tables.items()]
    head += [_segment(0xC4, b"".join(dht))] if one_dht else [_segment(0xC4, d) for d in dht]
    if dri:
        head.append(_segment(0xDD, dri.to_bytes(2, "big")))
    sos = bytes((len(comps),))
    for ci in range(len(comps)):
        sos += bytes((ids[ci], use[ci][0] << 4 | use[ci][1]))
    head.append(_segment(0xDA, sos + bytes((0, 63, 0))))
    pre = b"\xff" * fill
    out = b"\xff\xd8" + b"".join(pre + s for s in head) + bytes(w.out) + pre + b"\xff\xd9" + trailing
    _KNOWN[out] = q
    return out


# ------------------------------------------------------------------------------------------ the streams the tests share
@functools.lru_cache(maxsize=None)
def table_source(sampling):
    """27 x 43 (no multiple of any MCU), a different quality per sampling."""
    return source(27, 43, sampling, {"444": 100, "422": 90, "420": 60, "gray": 95}[sampling], seed=3)


@functools.lru_cache(maxsize=None)
def table_case(tset, assign, sampling):
    src = table_source(sampling)
    tables, use, one = assignment(assign, 1 if sampling == "gray" else 3, tset)
    return src, recode(src, tables, use, one_dht=one)


TABLE_CASES = [(t, a, s) for t in TABLE_SETS for a in ASSIGNMENTS for s in SAMPLINGS]


@functools.lru_cache(maxsize=None)
def restart_cases():
    """name -> (source, re-coded stream): 5 x 3 MCUs at 4:2:2 (33 x 70) and 3 x 5 at 4:2:0 (37 x 70)."""
    a, b = source(33, 70, "422", 85, seed=5), source(37, 70, "420", 75, seed=6)
    tiny = source(33, 70, "422", 12, seed=5, sigma=1.0)                   # every MCU codes to fewer than 16 bytes
    t = {(0, 0): UNARY_DC, (1, 0): SKEWED_AC, (0, 1): STD_DC, (1, 1): STD_AC}
    u = [(0, 0), (1, 1), (1, 1)]
    return {"dri1": (tiny, recode(tiny, dri=1)),                         # 25 segments: RSTn wraps three times
            "dri1_420": (b, recode(b, dri=1)),
            "dri7": (a, recode(a, t, u, dri=7)),                          # 25 MCUs: 7 + 7 + 7 + 4
            "dri_row": (a, recode(a, dri=5)),                             # one MCU row per segment
            "dri_row_420": (b, recode(b, t, u, dri=5)),
            "dri_all": (b, recode(b, dri=15)),                            # DRI == MCU count: one segment
            "dri_more": (b, recode(b, dri=1000)),
            "dri0": (a, recode(a, t, u))}


def dressing_cases():
    """name -> (source, dressed stream) for the stream-dressing cases; every one decodes to the source's pixels."""
    src = source(37, 53, "420", 80, seed=8)
    small = source(16, 24, "420", 50, seed=9)
    return {"fill": (src, recode(src, fill=3)),
            "com": (src, recode(src, com=b"a comment \xff\xd9 with an EOI inside", app=b"\x00\xff\xda\x01")),
            "fill_com": (src, recode(src, fill=2, com=b"abc")),
            "junk": (src, recode(src, trailing=b"\x00\x01\x02junk")),
            "second": (src, recode(src) + small),
            "second_dri": (src, recode(src, dri=2) + recode(small, dri=1)),
            "second_dri_first_plain": (src, recode(src) + recode(small, dri=1)),
            "nojfif": (src, recode(src, jfif=False)),
            "adobe1": (src, recode(src, jfif=False, adobe=1)),
            "ids012": (src, recode(src, ids=[0, 1, 2])),
            "sof1_dqt16": (src, recode(src, dqt16=True)),
            "one_dht": (src, recode(src, one_dht=True))}


GEOMETRY_SIZES = ((1, 1), (1, 50), (50, 1), (2, 2), (3, 3), (4, 12), (12, 4), (5, 5), (8, 8), (16, 16), (17, 17), (9, 1))


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """[(name, stream)]: every size x every sampling straight from Pillow, plus grayscale written with 2 x 2 factors."""
    out = []
    for k, (h, w) in enumerate(GEOMETRY_SIZES):
        for s in SAMPLINGS:
            d = source(h, w, s, 92, seed=20 + k)
            out.append((f"{h}x{w} {s}", d))
            if s == "gray":
                out.append((f"{h}x{w} gray2x2", recode(d, gray_factors=(2, 2))))
    return out


ALL_LIVE = dict(h=56, w=80, seed=4, sigma=34.0)        # chosen so that the flat-table stream fills all 1024 sub-sequences


@functools.lru_cache(maxsize=None)
def long_streams():
    """name -> (source, stream), all 4:4:4 at quality 100, one restart segment; seeds picked so that the conditions
    test_jpeg_streams_cpu.py::test_long_stream_input_conditions asserts hold:
      skewed_19k  45 x 70, skewed tables, about 20 KB: sub-sequences longer than the 128-bit minimum
      skewed_4k   24 x 32, skewed tables, just over one 4096-byte chunk of the un-stuffing kernel: 128-bit sub-sequences
      all_live    56 x 80, flat tables: ceil(8 * clean_len / sub_bits) == 1024 exactly
    Both skewed streams hold a stuffed FF 00 whose FF is the last byte of a 16-byte slice and one whose FF is the last byte of
    a 4096-byte chunk.  (A stream fills all 1024 sub-sequences only if fewer than sub_bits / 8 of its bytes are stuffed, which
    the skewed tables -- every long code starts with eight ones -- cannot give; the flat tables hardly ever stuff.)"""
    tables, use, _ = assignment("shared0", 3, "skewed")
    a = source(45, 70, "444", 100, seed=3, sigma=30)
    b = source(24, 32, "444", 100, seed=5)
    c = source(ALL_LIVE["h"], ALL_LIVE["w"], "444", 100, seed=ALL_LIVE["seed"], sigma=ALL_LIVE["sigma"])
    ft, fu, _ = assignment("shared0", 3, "flat")
    return {"skewed_19k": (a, recode(a, tables, use)), "skewed_4k": (b, recode(b, tables, use)), "all_live": (c, recode(c, ft, fu))}


@functools.lru_cache(maxsize=None)
def flat_stream():
    """Flat tables on every component, one segment: no code boundary re-synchronises a sub-sequence that started wrong."""
    return table_case("flat", "shared0", "444")


@functools.lru_cache(maxsize=None)
def undefined_ac_code_stream():
    """The flat-table stream with ONE scan byte changed so that the sequential decode meets an 8-bit AC code above 161, which
    the table leaves undefined.  Decided on the CPU: the oracle refuses the stream for its Huffman code, and no longer does
    once the AC table is completed to 256 codes -- so the first undefined code is an AC code."""
    _, data = flat_stream()
    j = J.parse_jpeg(data)
    start = data.index(j["scan"])
    full_ac = ([0] * 7 + [256] + [0] * 8, list(FLAT_AC[1]) + [0] * 94)
    for p in range(start + len(j["scan"]) // 2, start + len(j["scan"]) - 64):
        if 0xFF in data[p - 1:p + 2]:
            continue
        bad = data[:p] + b"\xa2" + data[p + 1:]
        jb = J.parse_jpeg(bad)
        try:
            J.decode_coefficients(jb)
            continue
        except J.JpegError as e:
            if "Huffman" not in str(e):
                continue
        jb["ht"][(1, 0)] = full_ac
        try:
            J.decode_coefficients(jb)
        except J.JpegError as e:
            if "Huffman" in str(e):
                continue
        return bad
    raise AssertionError("no byte of the flat stream gives an undefined AC code")


def stream_properties(data):
    """What the device decoder's launch geometry will be for a one-image batch of `data`, restated from the stream alone."""
    j = J.parse_jpeg(data)
    _, _, mcux, mcuy = J.geometry(j["frame"])
    raw = j["scan"]
    segments = 1 if not j["dri"] else -(-mcux * mcuy // j["dri"])
    clean = unstuff(raw)
    sub = max(128, (-(-len(raw) * 8 // 1024) + 31) & ~31)
    so = stuffed_offsets(raw)
    return dict(segments=segments, raw_len=len(raw), clean_len=len(clean), sub_bits=sub, live=-(-8 * len(clean) // sub),
                stuffed=len(so), stuffed_mod16_15=int((so % 16 == 15).sum()), stuffed_mod4096_4095=int((so % 4096 == 4095).sum()),
                first_mod16_15=int(so[so % 16 == 15][0]) if (so % 16 == 15).any() else None,
                first_mod4096_4095=int(so[so % 4096 == 4095][0]) if (so % 4096 == 4095).any() else None)


def unstuff(raw):
    return bytes(raw).replace(b"\xff\x00", b"\xff")


def stuffed_offsets(raw):
    """Offsets of every FF that a stuffed 00 follows."""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    return np.flatnonzero((a[:-1] == 0xFF) & (a[1:] == 0))
