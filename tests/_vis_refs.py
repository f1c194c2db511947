"""numpy restatements the visualisation tests compare against (no device, no product code):

  overlay_ref       skimage.color.label2rgb(kind="overlay", alpha=0.3, bg_label=0, image_alpha=1, saturation=0) followed by
                    matplotlib's float -> uint8 conversion, with a palette indexed by class instead of by rank
  jpeg_encode_ref   libjpeg's baseline encoder as Pillow drives it (`Image.save(buf, "JPEG", quality=q)`: 4:2:0, islow
                    integer DCT, the T.81 Annex K Huffman tables, no restart markers), markers included

`jpeg_encode_ref` takes three `fault_*` switches that plant the mistakes this arithmetic is easiest to get wrong; the CPU
tests check that each of them breaks the byte equality with Pillow, i.e. that the test images reach those code paths.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------------------- overlay
PALETTE_NAMES = ("red", "blue", "yellow", "magenta", "green", "indigo", "darkorange", "cyan", "pink", "yellowgreen")
PALETTE_RGB = np.array([(255, 0, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 128, 0), (75, 0, 130), (255, 140, 0),
                        (0, 255, 255), (255, 192, 203), (154, 205, 50)], dtype=np.uint8)      # the CSS colours of those names


def default_palette_ref():
    """uint8 [256, 3]: row 0 unused (label 0 is the grey image), row l = cycle colour (l - 1) % 10."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for l in range(1, 256):
        pal[l] = PALETTE_RGB[(l - 1) % 10]
    return pal


def overlay_ref(labels, rgb, palette=None, alpha=0.3):
    """labels uint8 (H, W), rgb uint8 (H, W, 3) -> uint8 (H, W, 3); float64, in the order the kernel documents."""
    pal = default_palette_ref() if palette is None else np.asarray(palette, dtype=np.uint8)
    rgb = np.asarray(rgb, dtype=np.float64)
    alpha = np.float64(alpha)
    g = (0.2125 * rgb[..., 0] + 0.7154 * rgb[..., 1] + 0.0721 * rgb[..., 2]) / 255
    lab = np.asarray(labels).astype(np.int64)
    col = pal[lab].astype(np.float64) / 255
    fg = (col * alpha + g[..., None] * (1 - alpha)) * 255
    bgv = np.repeat((g * 255)[..., None], 3, axis=2)
    out = np.where((lab > 0)[..., None], fg, bgv)
    return out.astype(np.uint8)               # truncation (values are >= 0)


# ---------------------------------------------------------------------------------------------------------- JPEG
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                       51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121,
                       120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# T.81 Annex K.3: (codes per length 1..16, symbols) for DC luminance, DC chrominance, AC luminance, AC chrominance
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def quant_table(base, quality):
    """jpeg_set_quality with force_baseline: natural-order int table."""
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(base, dtype=np.int64) * s + 50) // 100, 1, 255)


def huff_codes(counts, symbols):
    """T.81 Annex C canonical codes: symbol -> (code, length) as two int arrays of 256."""
    code = np.zeros(256, dtype=np.int64)
    size = np.zeros(256, dtype=np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            code[symbols[k]], size[symbols[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


def fdct_islow(b):
    """jfdctint.c (CONST_BITS 13, PASS1_BITS 2), rows first; b int64 [..., 8, 8] level-shifted samples -> 8 x the DCT."""
    C, P = 13, 2

    def D(x, n):
        return (x + (1 << (n - 1))) >> n

    def p(d, first):
        t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
        t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
        t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
        t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = [None] * 8
        if first:
            o[0], o[4], n = (t10 + t11) << P, (t10 - t11) << P, C - P
        else:
            o[0], o[4], n = D(t10 + t11, P), D(t10 - t11, P), C + P
        z1 = (t12 + t13) * 4433
        o[2], o[6] = D(z1 + t13 * 6270, n), D(z1 + t12 * (-15137), n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = z1 * (-7373), z2 * (-20995), z3 * (-16069) + z5, z4 * (-3196) + z5
        o[7], o[5], o[3], o[1] = D(t4 + z1 + z3, n), D(t5 + z2 + z4, n), D(t6 + z2 + z3, n), D(t7 + z1 + z4, n)
        return np.stack(o, -1)

    r = p(b, True)
    return p(r.swapaxes(-1, -2), False).swapaxes(-1, -2)


def quantise(c, q):
    q8 = np.asarray(q, dtype=np.int64).reshape(8, 8) * 8
    return np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)


def _blocks(plane, by, bx, q):
    """plane int64 [by*8, bx*8] samples -> quantised zig-zag blocks [by, bx, 64]."""
    blk = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128
    return quantise(fdct_islow(blk), q).reshape(by, bx, 64)[..., ZIGZAG]


def jpeg_coefficients_ref(rgb, quality=75, fault_bias=False, fault_rows=False, fault_dummy=False):
    """-> (Z int64 [n_mcu * 6, 64] quantised zig-zag blocks in scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU, dummy luma blocks
    filled in as libjpeg's compress_data does), luma table, chroma table)."""
    rgb = np.asarray(rgb)
    H, W, _ = rgb.shape
    r, g, b = [rgb[..., i].astype(np.int64) for i in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    ql, qc = quant_table(STD_LUMA_Q, quality), quant_table(STD_CHROMA_Q, quality)
    mcux, mcuy = -(-W // 16), -(-H // 16)
    bx, by = -(-W // 8), -(-H // 8)                   # real luma blocks
    yq = _blocks(np.pad(y, ((0, by * 8 - H), (0, bx * 8 - W)), mode="edge"), by, bx, ql)
    chroma = []
    ch = -(-H // 2)
    for pl in (cb, cr):
        if fault_rows:                               # edge-pad the full-resolution plane, then downsample
            pp = np.pad(pl, ((0, 16 * mcuy - H), (0, 16 * mcux - W)), mode="edge")
        else:                                        # pad columns, finish an odd row pair; missing rows come after downsampling
            pp = np.pad(pl, ((0, 2 * ch - H), (0, 16 * mcux - W)), mode="edge")
        bias = np.tile(np.array([2, 2] if fault_bias else [1, 2]), mcux * 4)[None, :]
        ds = (pp[0::2, 0::2] + pp[0::2, 1::2] + pp[1::2, 0::2] + pp[1::2, 1::2] + bias) >> 2
        ds = np.pad(ds, ((0, 8 * mcuy - ds.shape[0]), (0, 0)), mode="edge")
        chroma.append(_blocks(ds, mcuy, mcux, qc))
    Z = np.zeros((mcuy, mcux, 6, 64), dtype=np.int64)
    for my in range(mcuy):
        for mx in range(mcux):
            for yi in range(2):
                for xi in range(2):
                    Y, X, k = 2 * my + yi, 2 * mx + xi, 2 * yi + xi
                    if Y < by and X < bx:
                        Z[my, mx, k] = yq[Y, X]
                    elif not fault_dummy:            # AC 0, DC of the previous block in the MCU: right edge -> the block to
                        Z[my, mx, k, 0] = Z[my, mx, k - 1, 0] if Y < by else Z[my, mx, 1, 0]      # its left; bottom row -> block 1
            Z[my, mx, 4], Z[my, mx, 5] = chroma[0][my, mx], chroma[1][my, mx]
    return Z.reshape(-1, 64), ql, qc


def _category(v):
    a = np.abs(v)
    n = np.zeros(a.shape, dtype=np.int64)
    for k in range(16):
        n += (a >> k) > 0
    return n


def entropy_code_ref(Z):
    """T.81 F.1.2 sequential Huffman coding of the scan-ordered blocks -> (unstuffed bytes incl. the 1-padding, stuffed bytes)."""
    N = Z.shape[0]
    comp = np.arange(N) % 6                      # 0..3 luma, 4 Cb, 5 Cr
    is_c = comp >= 4
    dc = Z[:, 0]
    pred = np.zeros(N, dtype=np.int64)
    lum = np.flatnonzero(~is_c)
    pred[lum[1:]] = dc[lum[:-1]]
    for c in (4, 5):
        idx = np.flatnonzero(comp == c)
        pred[idx[1:]] = dc[idx[:-1]]
    diff = dc - pred
    tabs = {(0, 0): huff_codes(*DC_LUMA), (0, 1): huff_codes(*DC_CHROMA), (1, 0): huff_codes(*AC_LUMA), (1, 1): huff_codes(*AC_CHROMA)}

    def lookup(cls, chroma, sym):
        code = np.where(chroma, tabs[(cls, 1)][0][sym], tabs[(cls, 0)][0][sym])
        size = np.where(chroma, tabs[(cls, 1)][1][sym], tabs[(cls, 0)][1][sym])
        return code, size

    def extra(v, n):
        return np.where(v < 0, v - 1, v) & ((1 << n) - 1)

    keys, vals, lens = [], [], []
    # DC
    cat = _category(diff)
    code, size = lookup(0, is_c, cat)
    keys.append(np.arange(N) * 1024)
    vals.append((code << cat) | extra(diff, cat))
    lens.append(size + cat)
    # AC
    blk, pos = np.nonzero(Z[:, 1:])
    pos = pos + 1
    prev = np.zeros_like(pos)
    same = np.zeros(len(pos), dtype=bool)
    same[1:] = blk[1:] == blk[:-1]
    prev[1:] = np.where(same[1:], pos[:-1], 0)
    run = pos - prev - 1
    v = Z[blk, pos]
    n = _category(v)
    code, size = lookup(1, is_c[blk], ((run & 15) << 4) | n)
    keys.append(blk * 1024 + pos * 4 + 3)
    vals.append((code << n) | extra(v, n))
    lens.append(size + n)
    for j in range(3):                           # ZRL: one 0xF0 per 16 zeros of the run
        m = (run >> 4) > j
        code, size = lookup(1, is_c[blk[m]], np.full(int(m.sum()), 0xF0))
        keys.append(blk[m] * 1024 + pos[m] * 4 + j)
        vals.append(code)
        lens.append(size)
    last = np.zeros(N, dtype=np.int64)
    np.maximum.at(last, blk, pos)
    eob = np.flatnonzero(last < 63)
    code, size = lookup(1, is_c[eob], np.zeros(len(eob), dtype=np.int64))
    keys.append(eob * 1024 + 64 * 4)
    vals.append(code)
    lens.append(size)
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    vals, lens = vals[order], lens[order]
    bits = ((vals[:, None] >> np.arange(31, -1, -1)[None, :]) & 1).astype(np.uint8)
    keep = np.arange(32)[None, :] >= (32 - lens)[:, None]
    stream = bits[keep]
    padn = (-len(stream)) % 8
    stream = np.concatenate([stream, np.ones(padn, dtype=np.uint8)])
    raw = np.packbits(stream)
    out = np.zeros(2 * len(raw), dtype=np.uint8)
    ff = raw == 0xFF
    at = np.arange(len(raw)) + np.concatenate([[0], np.cumsum(ff)[:-1]])
    out[at] = raw
    return raw.tobytes(), out[: len(raw) + int(ff.sum())].tobytes()


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def jpeg_headers_ref(H, W, ql, qc):
    """SOI, APP0 (JFIF 1.01, no density), DQT 0, DQT 1, SOF0 (2x2, 1x1, 1x1), DHT DC0 AC0 DC1 AC1, SOS."""
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _seg(0xDB, bytes([0]) + bytes(int(v) for v in np.asarray(ql)[ZIGZAG]))
    out += _seg(0xDB, bytes([1]) + bytes(int(v) for v in np.asarray(qc)[ZIGZAG]))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (counts, syms) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, bytes([tc_th]) + bytes(counts) + bytes(syms))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def jpeg_encode_ref(rgb, quality=75, **faults):
    rgb = np.asarray(rgb)
    Z, ql, qc = jpeg_coefficients_ref(rgb, quality, **faults)
    return jpeg_headers_ref(int(rgb.shape[0]), int(rgb.shape[1]), ql, qc) + entropy_code_ref(Z)[1] + b"\xff\xd9"


def pillow_jpeg(rgb, quality=75):
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb, dtype=np.uint8)).save(b, "JPEG", quality=int(quality))
    return b.getvalue()


# ---------------------------------------------------------------------------------------------------------- test images
SIZES = ((1, 1), (8, 8), (16, 16), (24, 40), (40, 24), (37, 29), (9, 50), (17, 33), (375, 500))
CONTENTS = ("smooth", "noise", "black", "white", "checker")


def test_image(kind, H, W, seed=0):
    """smooth: 4 x 4 colour patches + noise of +-6; noise: uniform (many stuffed 0xFF bytes, long codes); black / white: DC-only
    blocks; checker: a flat black field with one 8 x 8 block of 128 +- 127 in 4 x 4 cells in the top-left corner -- at quality 95
    its AC coefficients reach 834 (size 10, the largest AC category) and the DC step to the field is 512 (size 10: the luma DC
    table of quality <= 95 divides by 2 at least, so |difference| <= 1020 and size 11 cannot occur in a Pillow file).  ZRL runs
    come with the smooth and the noise images."""
    rng = np.random.default_rng(seed + 7 * H + W)
    if kind == "smooth":
        base = rng.integers(0, 256, (H // 4 + 1, W // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:H, :W]
        return np.clip(base + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "black":
        return np.zeros((H, W, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((H, W, 3), 255, dtype=np.uint8)
    if kind == "checker":
        img = np.zeros((H, W, 3), dtype=np.int64)
        yy, xx = np.mgrid[0:min(H, 8), 0:min(W, 8)]
        img[:min(H, 8), :min(W, 8)] = 128 + np.where((yy // 4 + xx // 4) % 2 == 0, 127, -127)[..., None]
        return img.astype(np.uint8)
    raise ValueError(kind)


# the truncation witness of the overlay: grey of (255, 255, 0) is 0.9279 * 255 = 236.6145 -> 236 truncated, 237 rounded
TRUNCATION_WITNESS_RGB = (255, 255, 0)
