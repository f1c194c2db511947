"""Reference for the label-map PNG files (csrc/png_enc.hip + pnp_ovss/png.py): a pure-Python encoder of the normative byte
format, written from its description, RFC 1950 / 1951 and the PNG specification -- it imports nothing of the package.

Format.  Signature; IHDR (8-bit, colour type 3 with a palette / 0 without, no interlace); PLTE (256 entries, colour type 3 only);
one IDAT; IEND.  The IDAT payload is a zlib stream: 78 01, ONE deflate block (BFINAL = 1, BTYPE = 01: the fixed Huffman code),
end-of-block, zero bits to a whole byte, Adler-32 of the filtered stream (big-endian).
Filtered stream: for row y, R = the W label bytes, U[x] = (R_y[x] - R_{y-1}[x]) mod 256 (R_{-1} = 0); c0 / c2 = the number of x in
1..W-1 where R / U differs from its left neighbour; the row is (2, U) if c2 < c0, else (0, R).
Tokens: the W + 1 bytes of a row are cut into maximal runs of equal bytes (never across rows); a run of byte b, length r:
literal b; (r - 1) // 258 matches of length 258, distance 1; t = (r - 1) % 258: one match of length t if t >= 3, else t literals.
"""
import struct
import zlib

import numpy as np

# RFC 1951 3.2.5: length codes 257..285 -> (base length, extra bits)
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def filtered_stream(labels, force=None):
    """-> (bytes of the filtered stream, [filter byte per row]).  force: 0 / 2 for every row instead of the per-row choice
    (row 0 under Up equals row 0 under None but for the filter byte)."""
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    H, W = lab.shape
    out, filters = bytearray(), []
    prev = np.zeros(W, dtype=np.uint8)
    for y in range(H):
        R = lab[y]
        U = (R.astype(np.int32) - prev.astype(np.int32)).astype(np.uint8)       # mod 256
        c0 = int(np.count_nonzero(R[1:] != R[:-1]))
        c2 = int(np.count_nonzero(U[1:] != U[:-1]))
        f = (2 if c2 < c0 else 0) if force is None else force
        out.append(f)
        out += (U if f == 2 else R).tobytes()
        filters.append(f)
        prev = R
    return bytes(out), filters


def tokens_of(stream, H, W):
    """-> [("lit", b) | ("match", length)]: every match is at distance 1."""
    toks = []
    L = W + 1
    for y in range(H):
        row = stream[y * L:(y + 1) * L]
        i = 0
        while i < L:
            j = i
            while j < L and row[j] == row[i]:
                j += 1
            b, rem = row[i], j - i - 1
            toks.append(("lit", b))
            toks += [("match", 258)] * (rem // 258)
            t = rem % 258
            toks += [("match", t)] if t >= 3 else [("lit", b)] * t
            i = j
    return toks


class _Bits:
    """deflate's bit order: bits fill a byte from its least significant end."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):                   # a field with its least significant bit first (header, extra bits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_huffman(self, code, nbits):            # a Huffman code: most significant bit first
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def flush(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _put_litlen(bw, sym):
    """RFC 1951 3.2.6: 0..143 -> 8 bits from 00110000; 144..255 -> 9 bits from 110010000; 256..279 -> 7 bits from 0000000;
    280..287 -> 8 bits from 11000000."""
    if sym < 144:
        bw.put_huffman(0x30 + sym, 8)
    elif sym < 256:
        bw.put_huffman(0x190 + sym - 144, 9)
    elif sym < 280:
        bw.put_huffman(sym - 256, 7)
    else:
        bw.put_huffman(0xC0 + sym - 280, 8)


def deflate_fixed(toks):
    bw = _Bits()
    bw.put(1, 1)                                   # BFINAL
    bw.put(1, 2)                                   # BTYPE = 01
    for kind, v in toks:
        if kind == "lit":
            _put_litlen(bw, v)
        else:
            c = max(k for k in range(29) if _LEN_BASE[k] <= v)
            _put_litlen(bw, 257 + c)
            bw.put(v - _LEN_BASE[c], _LEN_EXTRA[c])
            bw.put_huffman(0, 5)                   # distance code 0: distance 1, no extra bits
    _put_litlen(bw, 256)
    return bw.flush()


def adler32(data):
    a, b = 1, 0
    for v in data:
        a = (a + v) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def zlib_stream(labels, force=None):
    """-> (zlib stream, filtered stream, tokens)."""
    lab = np.asarray(labels)
    filt, _ = filtered_stream(lab, force)
    toks = tokens_of(filt, lab.shape[0], lab.shape[1])
    return b"\x78\x01" + deflate_fixed(toks) + struct.pack(">I", adler32(filt)), filt, toks


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_file(H, W, stream, palette):
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if palette is None else 3, 0, 0, 0))
    if palette is not None:
        out += _chunk(b"PLTE", np.ascontiguousarray(palette, dtype=np.uint8).tobytes())
    return out + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


def encode(labels, palette=None, force=None):
    """-> (filtered stream, token list, file bytes) of one (H, W) uint8 label map."""
    lab = np.asarray(labels)
    stream, filt, toks = zlib_stream(lab, force)
    return filt, toks, png_file(lab.shape[0], lab.shape[1], stream, palette)


def stream_capacity_ref(H, W):
    n = H * (W + 1)
    return 2 + -(-(10 + 9 * n) // 8) + 4


def voc_palette_ref():
    """The PASCAL VOC devkit's colormap: bits 0, 1, 2 of the class index go to R, G, B from the top bit down, three at a time."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c = i
        for j in range(8):
            pal[i, 0] |= ((c >> 0) & 1) << (7 - j)
            pal[i, 1] |= ((c >> 1) & 1) << (7 - j)
            pal[i, 2] |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
    return pal


def blob_map(H, W, classes, seed):
    """A label map like a post-CRF one: `classes` labels (0 = background) in a few smooth regions -- every pixel takes the label
    of the strongest of `classes` random Gaussian bumps."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    best = np.full((H, W), -np.inf)
    lab = np.zeros((H, W), dtype=np.uint8)
    for k in range(classes):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        s = rng.uniform(0.15, 0.45) * max(H, W)
        v = rng.uniform(0.6, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        if k == 0:
            v = np.full((H, W), 0.35)              # the background: wherever no bump is strong
        lab[v > best] = k
        best = np.maximum(best, v)
    return lab


def all_literal_stream(H, W):
    """H * (W + 1) stream bytes of which no two neighbours are equal and every one is >= 144: the token layer's worst case,
    all 9-bit literals.  (A real filtered stream stays H bits below it: its filter bytes, 0 or 2, are 8-bit literals.)"""
    n = H * (W + 1)
    return bytes(144 + (7 * i) % 112 for i in range(n))


def stream_of_filtered(filt, H, W):
    """The zlib stream around an already filtered stream of H rows of W + 1 bytes."""
    return b"\x78\x01" + deflate_fixed(tokens_of(filt, H, W)) + struct.pack(">I", adler32(filt))
