"""Label maps as 8-bit PNG files: the host half.  The device writes the zlib stream of the IDAT chunk (csrc/png_enc.hip through
hip.png_encode_batch); this module writes the chunks around it -- signature, IHDR, PLTE for an indexed file, one IDAT, IEND --
and their CRC-32 (zlib.crc32: the stream is a few KB and the host holds it anyway).  No device, no torch: importable anywhere.

A file is colour type 3 (one byte per pixel + a 256-entry palette: what the VOC / ADE20K evaluation servers, mmseg-style
evaluators and annotation viewers read) or, without a palette, colour type 0 (8-bit grey)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 65535                       # pnp_png_encode's limit on H and W
MAX_STREAM_BYTES = (1 << 31) // 9      # filtered-stream bytes (the sum of H * (W + 1)) per pnp_png_encode call: int32 bit offsets


def stream_capacity(H, W):
    """The longest zlib stream pnp_png_encode can write for an H x W map: every byte of the filtered stream a 9-bit literal,
    10 bits of block header and end-of-block, the 2-byte zlib header and the 4-byte Adler-32."""
    n = int(H) * (int(W) + 1)
    return 2 + (10 + 9 * n + 7) // 8 + 4


def voc_palette():
    """The PASCAL VOC colormap (the public bit-interleave rule of the devkit's VOClabelcolormap), uint8 [256, 3]: bit k of
    class c goes to bit 7 - k // 3 of channel k % 3."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        pal[i] = rgb
    return pal


def resolve_palette(palette):
    """"voc" -> voc_palette(); "overlay" -> the colours pnp_ovss.vis gives each class; "grey" / None -> None (colour type 0);
    anything else: a (256, 3) uint8 array."""
    if palette is None or (isinstance(palette, str) and palette == "grey"):
        return None
    if isinstance(palette, str):
        if palette == "voc":
            return voc_palette()
        if palette == "overlay":
            from .vis import default_palette
            return default_palette()
        raise ValueError(f"unknown palette {palette!r}: voc, overlay, grey, None or a (256, 3) uint8 array")
    pal = np.asarray(palette)
    if pal.shape != (256, 3) or pal.dtype != np.uint8:
        raise ValueError(f"a palette is a (256, 3) uint8 array, not {pal.shape} {pal.dtype}")
    return np.ascontiguousarray(pal)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_chunks(H, W, zlib_stream, palette):
    """The PNG file of an H x W 8-bit image whose IDAT payload is `zlib_stream`: colour type 3 with `palette` ((256, 3) uint8),
    colour type 0 with palette None.  No interlace; one IDAT chunk."""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image sizes are 1..{MAX_SIDE}, not {H} x {W}")
    pal = resolve_palette(palette)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if pal is None else 3, 0, 0, 0))]
    if pal is not None:
        out.append(_chunk(b"PLTE", pal.tobytes()))
    out.append(_chunk(b"IDAT", bytes(zlib_stream)))
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)
