"""BC1 / BC3 / BC5 in numpy, written from the text of include/ptx.h (PtxTextureFormat) and from nothing else: block layout,
palette rules, the upload rules' budget in block bytes.  It shares no code with TextureImporter::DecodeDds or with
csrc/pt_bc.hpp, so neither the host decoder nor the kernel can share a mistake with it."""
import struct

import numpy as np

BC1_UNORM, BC1_SRGB, BC3_SRGB, BC5_UNORM = 3, 4, 5, 6
RGBA8_UNORM, RGBA8_SRGB = 0, 1
BLOCK_BYTES = {BC1_UNORM: 8, BC1_SRGB: 8, BC3_SRGB: 16, BC5_UNORM: 16}
TWIN_FORMAT = {BC1_UNORM: RGBA8_UNORM, BC1_SRGB: RGBA8_SRGB, BC3_SRGB: RGBA8_SRGB, BC5_UNORM: RGBA8_UNORM}


def mip_dim(v, l):
    return max(v >> l, 1)


def full_levels(w, h):
    return int(np.floor(np.log2(max(w, h)))) + 1


def level_blocks(w, h, l):
    return ((mip_dim(w, l) + 3) // 4) * ((mip_dim(h, l) + 3) // 4)


def chain_bytes(w, h, levels, fmt, first=0):
    """Bytes of the levels [first, first + levels) of a w x h image."""
    return sum(level_blocks(w, h, l) for l in range(first, first + levels)) * BLOCK_BYTES[fmt]


def max_extent(fmt, share):
    """The largest square power-of-two extent (from 4096 down) whose full chain fits `share` bytes.  fmt: a BC format, or
    RGBA8 (4 B per texel)."""
    m = 4096
    while m > 1:
        if fmt in BLOCK_BYTES:
            size = chain_bytes(m, m, full_levels(m, m), fmt)
        else:
            size = 4 * sum(mip_dim(m, l) * mip_dim(m, l) for l in range(full_levels(m, m)))
        if size <= share:
            break
        m >>= 1
    return m


def _colour_block(b, punch_through):
    """b: (n, 8) uint8 -> (n, 16, 4) uint8 RGBA."""
    b = b.astype(np.int64)
    c0 = b[:, 0] | b[:, 1] << 8
    c1 = b[:, 2] | b[:, 3] << 8
    codes = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24

    def expand(c):
        r, g, bl = (c >> 11) & 31, (c >> 5) & 63, c & 31
        return np.stack([r << 3 | r >> 2, g << 2 | g >> 4, bl << 3 | bl >> 2], -1)

    p0, p1 = expand(c0), expand(c1)
    four = (c0 > c1) if punch_through else np.ones(len(b), bool)
    pal = np.zeros((len(b), 4, 4), np.int64)
    pal[:, 0, :3], pal[:, 1, :3] = p0, p1
    pal[:, :, 3] = 255
    f = four[:, None]
    pal[:, 2, :3] = np.where(f, (2 * p0 + p1) // 3, (p0 + p1) // 2)
    pal[:, 3, :3] = np.where(f, (p0 + 2 * p1) // 3, 0)
    pal[:, 3, 3] = np.where(four, 255, 0)
    i = np.arange(16)
    code = (codes[:, None] >> (2 * i)[None, :]) & 3
    return pal[np.arange(len(b))[:, None], code].astype(np.uint8)


def _alpha_block(b):
    """b: (n, 8) uint8 -> (n, 16) uint8."""
    b = b.astype(np.int64)
    a0, a1 = b[:, 0], b[:, 1]
    bits = np.zeros(len(b), np.int64)
    for k in range(6):
        bits |= b[:, 2 + k] << (8 * k)
    pal = np.zeros((len(b), 8), np.int64)
    pal[:, 0], pal[:, 1] = a0, a1
    eight = a0 > a1
    for c in range(2, 8):
        v8 = ((8 - c) * a0 + (c - 1) * a1) // 7
        v6 = ((6 - c) * a0 + (c - 1) * a1) // 5 if c <= 5 else np.full(len(b), 0 if c == 6 else 255)
        pal[:, c] = np.where(eight, v8, v6)
    i = np.arange(16)
    code = (bits[:, None] >> (3 * i)[None, :]) & 7
    return pal[np.arange(len(b))[:, None], code].astype(np.uint8)


def decode_level(blocks, w, h, fmt):
    """One level: `blocks` = ceil(w / 4) * ceil(h / 4) blocks, row-major -> (h, w, 4) uint8."""
    bw, bh = (w + 3) // 4, (h + 3) // 4
    nb = BLOCK_BYTES[fmt]
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(bw * bh, nb)
    if fmt in (BC1_UNORM, BC1_SRGB):
        px = _colour_block(b, True)
    elif fmt == BC3_SRGB:
        px = _colour_block(b[:, 8:], False)
        px[:, :, 3] = _alpha_block(b[:, :8])
    else:
        px = np.zeros((bw * bh, 16, 4), np.uint8)
        px[:, :, 0], px[:, :, 1], px[:, :, 3] = _alpha_block(b[:, :8]), _alpha_block(b[:, 8:]), 255
    # texel i = 4 (y & 3) + (x & 3) of block (bx, by)
    img = px.reshape(bh, bw, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)
    return np.ascontiguousarray(img[:h, :w])


def decode_chain(data, w, h, levels, fmt, first=0):
    """The levels [first, levels) of a file of `levels` levels -> list of (h_l, w_l, 4) uint8."""
    data = bytes(data)
    out, offset = [], 0
    for l in range(levels):
        n = level_blocks(w, h, l) * BLOCK_BYTES[fmt]
        if l >= first:
            out.append(decode_level(data[offset:offset + n], mip_dim(w, l), mip_dim(h, l), fmt))
        offset += n
    assert offset == len(data), (offset, len(data))
    return out


def twin_texels(data, w, h, levels, fmt, first=0):
    """The RGBA8 twin's flat texel array: the decoded levels back to back."""
    return np.concatenate([lv.reshape(-1) for lv in decode_chain(data, w, h, levels, fmt, first)])


def random_blocks(rng, w, h, levels, fmt):
    """Random bytes are valid blocks and reach both modes of every palette."""
    return rng.integers(0, 256, chain_bytes(w, h, levels, fmt), dtype=np.uint8)


def crafted_colour_blocks():
    """8-byte colour blocks: equal end points, c0 == c1 with every code, punch-through on every index, all-0 and all-1 index bits
    in both orders of the end points."""
    out = []
    for c0, c1 in ((0x1234, 0x1234), (0xffff, 0xffff), (0x0000, 0x0000), (0xf81f, 0x07e0), (0x07e0, 0xf81f), (0x8410, 0x8411), (0x8411, 0x8410)):
        for codes in (0x00000000, 0xffffffff, 0x55555555, 0xaaaaaaaa, 0xe4e4e4e4, 0x1b1b1b1b):
            out.append(struct.pack("<HHI", c0, c1, codes))
    return out


def crafted_alpha_blocks():
    """8-byte alpha blocks: a0 == a1, both orders, the extremes, all-0 and all-1 code bits and every code."""
    every = sum((i % 8) << (3 * i) for i in range(16))
    out = []
    for a0, a1 in ((77, 77), (0, 0), (255, 255), (255, 0), (0, 255), (200, 13), (13, 200), (128, 127), (127, 128)):
        for bits in (0, (1 << 48) - 1, every, every ^ ((1 << 48) - 1)):
            out.append(bytes([a0, a1]) + bits.to_bytes(6, "little"))
    return out


def crafted_blocks(fmt, count, rng):
    """`count` blocks of the format: the crafted ones first (combined pairwise for the 16-byte formats), random bytes behind."""
    colour, alpha = crafted_colour_blocks(), crafted_alpha_blocks()
    if fmt in (BC1_UNORM, BC1_SRGB):
        made = colour
    elif fmt == BC3_SRGB:
        made = [alpha[k % len(alpha)] + colour[k % len(colour)] for k in range(max(len(alpha), len(colour)))]
    else:
        made = [alpha[k] + alpha[(5 * k + 3) % len(alpha)] for k in range(len(alpha))]
    buf = np.frombuffer(b"".join(made), np.uint8)
    need = count * BLOCK_BYTES[fmt]
    if len(buf) >= need:
        return buf[:need].copy()
    return np.concatenate([buf, rng.integers(0, 256, need - len(buf), dtype=np.uint8)])


def dds_file(data, w, h, levels, fmt, dx10=False):
    """A DDS file around the blocks: the legacy header with the FourCC, or the DX10 extension."""
    four_cc = b"DX10" if dx10 else {8: b"DXT1"}.get(BLOCK_BYTES[fmt], b"DXT5" if fmt == BC3_SRGB else b"ATI2")
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | (0x20000 if levels > 1 else 0)
    hdr = struct.pack("<4s7I44x", b"DDS ", 124, flags, h, w, 0, 0, levels)
    hdr += struct.pack("<2I4s5I", 32, 0x4, four_cc, 0, 0, 0, 0, 0) + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    assert len(hdr) == 128, len(hdr)
    if dx10:
        dxgi = {BC1_UNORM: 71, BC1_SRGB: 72, BC3_SRGB: 78, BC5_UNORM: 83}[fmt]
        hdr += struct.pack("<5I", dxgi, 3, 0, 1, 0)
    return hdr + bytes(data)
