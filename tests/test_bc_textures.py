"""Block-compressed scene textures (docs/NEXT_ROWS.md section 15): BC1 / BC3 / BC5 uploaded as blocks and decoded on the device.

The reference of every GPU test is the oracle on the RGBA8 TWIN: the same description with the blocks decoded by tests/bc_ref.py
(numpy, written from the text of include/ptx.h), format RGBA8_SRGB / RGBA8_UNORM, the same `levels`.  The oracle never sees a
format 3 .. 6.  Everything is compared bit for bit."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import bc_ref
from bc_ref import BC1_SRGB, BC1_UNORM, BC3_SRGB, BC5_UNORM, RGBA8_SRGB, RGBA8_UNORM
from test_texture_streaming import _same, _stand_in_desc, _stand_ins_by_type, _textures, _with_textures

FORMATS = (BC1_UNORM, BC1_SRGB, BC3_SRGB, BC5_UNORM)
NO_LIMIT = 2**64 - 1
# the per-texture share of test_textures._BUDGET_32: RGBA8 keeps 32 x 32 (chain of 32: 5,460 B, of 64: 21,844 B), every BC
# format keeps 64 x 64 (chain of 64: 2,744 / 5,488 B, of 128: 10,936 / 21,872 B)
SHARE = 6000
WHITE = np.array([0xFFFFFFFF], "<u4")


def _inputs(idx, u, v, dudx=0.0, dvdx=0.0, dudy=0.0, dvdy=0.0):
    a = np.zeros((len(u), 7), np.float32)
    a.view(np.uint32)[:, 0] = idx
    a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5], a[:, 6] = u, v, dudx, dvdx, dudy, dvdy
    return a


def _lookups(seed, n, first, last):
    rng = np.random.default_rng(seed)
    idx = rng.integers(first, last, n).astype(np.uint32)
    uv = rng.uniform(-1.5, 2.5, (n, 2)).astype(np.float32)
    g = (10.0 ** rng.uniform(-4, 0.3, (n, 4)) * rng.choice([-1, 1], (n, 4))).astype(np.float32)
    g[:50] = 0
    return _inputs(idx, uv[:, 0], uv[:, 1], g[:, 0], g[:, 1], g[:, 2], g[:, 3])


class _Tex:
    """One texture of a test: (w, h, format, levels, flat uint8 data) and, for a BC one, its RGBA8 twin."""

    def __init__(self, w, h, fmt, levels, data):
        self.w, self.h, self.fmt, self.levels, self.data = w, h, fmt, levels, np.ascontiguousarray(data)

    def desc(self, pkg, data=True):
        return pkg.TextureDesc(self.w, self.h, self.fmt, self.levels, self.data.ctypes.data if data else None)

    def twin(self, first=0):
        """The RGBA8 twin: the levels from `first` on, decoded by bc_ref."""
        if self.fmt not in bc_ref.BLOCK_BYTES:
            return self
        texels = bc_ref.twin_texels(self.data, self.w, self.h, self.levels, self.fmt, first)
        return _Tex(bc_ref.mip_dim(self.w, first), bc_ref.mip_dim(self.h, first), bc_ref.TWIN_FORMAT[self.fmt], self.levels - first, texels)


def _white():
    return _Tex(1, 1, RGBA8_UNORM, 1, WHITE.view(np.uint8))


def _bc(rng, w, h, fmt, levels=None, crafted=False):
    levels = bc_ref.full_levels(w, h) if levels is None else levels
    if crafted:
        n = bc_ref.chain_bytes(w, h, levels, fmt) // bc_ref.BLOCK_BYTES[fmt]
        return _Tex(w, h, fmt, levels, bc_ref.crafted_blocks(fmt, n, rng))
    return _Tex(w, h, fmt, levels, bc_ref.random_blocks(rng, w, h, levels, fmt))


def _desc(pkg, scene_desc, texs, budget=NO_LIMIT, force_full=False):
    d, keep = _with_textures(pkg, scene_desc, [t.desc(pkg) for t in texs], budget=budget)
    d.forceFullTextureSize = 1 if force_full else 0
    return d, (keep, texs)


def _status(excinfo):
    return int(re.match(r"status (\d+)", str(excinfo.value)).group(1))


# ---------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------
def test_header_enum_export_and_bindings(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    for name, value in (("PTX_TEXTURE_BC1_UNORM", 3), ("PTX_TEXTURE_BC1_SRGB", 4), ("PTX_TEXTURE_BC3_SRGB", 5), ("PTX_TEXTURE_BC5_UNORM", 6)):
        assert re.search(rf"\b{name} = {value}\b", header), name
    assert (pkg.TEXTURE_BC1_UNORM, pkg.TEXTURE_BC1_SRGB, pkg.TEXTURE_BC3_SRGB, pkg.TEXTURE_BC5_UNORM) == (3, 4, 5, 6)
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header
    assert re.search(r"PTX_API uint32_t ptx_textures_rejected\(PtxRenderer \*r, uint32_t \*indices, uint32_t capacity\);", header)
    # the layout and the rules are stated as text: bc_ref is written from them
    for phrase in ("4 (y & 3) + (x & 3)", "(2 p0 + p1) / 3", "(p0 + p1) / 2", "((8 - c) a0 + (c - 1) a1) / 7", "((6 - c) a0 + (c - 1) a1) / 5",
                   "four-colour mode iff c0 > c1", "skip = levels - fullLevels(w', h')", "REJECTED"):
        assert phrase in header, phrase
    assert "ptx_textures_rejected" in pkg.PTX_SYMBOLS and hasattr(pkg.Renderer, "textures_rejected")
    assert hasattr(pkg.load_hip(), "ptx_textures_rejected")
    host = open(os.path.join(pkg.REPO_DIR, "include", "ptx_host.h")).read()
    assert "PTH_SCENE_NATIVE_BC = 1u" in host and "pth_scene_create_ex" in pkg.PTH_SYMBOLS and hasattr(pkg.load_host(), "pth_scene_create_ex")
    assert open(os.path.join(pkg.REPO_DIR, "path-tracing_amd", "csrc", "pt_bc.hpp")).read().count("k_decode_bc") >= 1


@pytest.mark.parametrize("fmt", (BC1_SRGB, BC3_SRGB, BC5_UNORM))
@pytest.mark.parametrize("shape", ((4, 4), (5, 3), (8, 8), (67, 45), (64, 64), (256, 4), (1, 1)))
def test_bc_ref_matches_the_host_decoder(pkg, fmt, shape):
    """Two independent decoders, one answer: bc_ref on the blocks, pkg.decode_image_levels on a DDS file around them --
    crafted blocks first, random bytes behind, with the file's own chain, both header flavours."""
    w, h = shape
    rng = np.random.default_rng(w * 131 + h * 7 + fmt)
    t = _bc(rng, w, h, fmt, crafted=True)
    for dx10 in (False, True):
        levels = pkg.decode_image_levels(bc_ref.dds_file(t.data, w, h, t.levels, fmt, dx10))
        mine = bc_ref.decode_chain(t.data, w, h, t.levels, fmt)
        assert len(levels) == len(mine) == t.levels
        for a, b in zip(levels, mine):
            assert a.shape == b.shape and (np.asarray(a) == b).all()


def test_bc_ref_known_answers():
    """The four cases of test_decoders.test_block_compressed_dds, by hand."""
    c0, c1 = 0xF800, 0x001F
    img = bc_ref.decode_level(struct.pack("<HHI", c0, c1, 0xE4E4E4E4), 4, 4, BC1_UNORM)
    assert img[0].tolist() == [[255, 0, 0, 255], [0, 0, 255, 255], [170, 0, 85, 255], [85, 0, 170, 255]]
    assert (bc_ref.decode_level(struct.pack("<HHI", c1, c0, 0xFFFFFFFF), 4, 4, BC1_SRGB) == 0).all()
    # c0 == c1 is three-colour mode: code 2 is the end point itself, code 3 transparent black
    img = bc_ref.decode_level(struct.pack("<HHI", 0x07E0, 0x07E0, 0xFFFFAAAA), 4, 4, BC1_UNORM)
    assert (img[:2] == [0, 255, 0, 255]).all() and (img[2:] == 0).all()
    alpha = bytes([200, 100]) + (0o1010101010101010).to_bytes(6, "little")
    img = bc_ref.decode_level((alpha + struct.pack("<HHI", 0x07E0, 0x07E0, 0)) * 2, 5, 3, BC3_SRGB)
    assert img.shape == (3, 5, 4) and (img[..., 1] == 255).all() and set(np.unique(img[..., 3])) == {100, 200}
    # BC3's colour block never punches through, whatever the order of its end points
    img = bc_ref.decode_level(bytes([9, 9] + [0] * 6) + struct.pack("<HHI", c1, c0, 0xFFFFFFFF), 4, 4, BC3_SRGB)
    assert (img == [(0 + 2 * 255) // 3, 0, (255 + 0) // 3, 9]).all()
    r = bytes([10, 250]) + (0).to_bytes(6, "little")
    g = bytes([250, 10]) + ((1 << 48) - 1).to_bytes(6, "little")
    img = bc_ref.decode_level(r + g, 4, 4, BC5_UNORM)
    assert (img[..., 0] == 10).all() and (img[..., 1] == (1 * 250 + 6 * 10) // 7).all() and (img[..., 2] == 0).all() and (img[..., 3] == 255).all()
    # six-value mode: codes 6 and 7 are 0 and 255
    six = bytes([10, 250]) + sum(c << (3 * i) for i, c in enumerate([6, 7, 2, 5] * 4)).to_bytes(6, "little")
    assert bc_ref.decode_level(six + six, 4, 4, BC5_UNORM)[0, :, 0].tolist() == [0, 255, (4 * 10 + 250) // 5, (10 + 4 * 250) // 5]


def test_budget_in_block_bytes():
    assert bc_ref.chain_bytes(64, 64, 7, BC1_UNORM) == 2744 and bc_ref.chain_bytes(128, 128, 8, BC1_SRGB) == 10936
    assert bc_ref.chain_bytes(64, 64, 7, BC3_SRGB) == 5488 and bc_ref.chain_bytes(128, 128, 8, BC5_UNORM) == 21872
    assert bc_ref.chain_bytes(64, 64, 7, BC1_UNORM) // 8 == 343 and bc_ref.chain_bytes(128, 128, 8, BC1_UNORM) // 8 == 1367
    assert bc_ref.max_extent(RGBA8_UNORM, SHARE) == 32
    assert [bc_ref.max_extent(f, SHARE) for f in FORMATS] == [64, 64, 64, 64]
    # BC1 keeps 8x, BC3 / BC5 4x the texels of RGBA8 under one share
    assert bc_ref.max_extent(BC1_SRGB, 21844) == 128 and bc_ref.max_extent(BC3_SRGB, 21844) == 64 and bc_ref.max_extent(RGBA8_SRGB, 21844) == 64
    assert bc_ref.max_extent(BC1_UNORM, 2000) == 32  # chain of 32: 87 blocks, 696 B


def _dds_scene(tmp_path, materials):
    """A glTF with one quad per material = (base colour file, normal map file or None); every image an external .dds."""
    from gltf_util import GltfWriter, quad

    w = GltfWriter()
    pos, nrm, uv, idx = quad()
    for k, (colour, normal) in enumerate(materials):
        fields = {"pbrMetallicRoughness": {"baseColorTexture": {"index": w.image_texture(colour, "uri", tmp_path, f"c{k}.dds")}}}
        if normal is not None:
            fields["normalTexture"] = {"index": w.image_texture(normal, "uri", tmp_path, f"n{k}.dds")}
        m = w.material(name=f"M{k}", **fields)
        w.node(mesh=w.mesh([w.primitive(pos + np.float32([2.5 * k, 0, 0]), idx, nrm, uv, material=m)]))
    path = tmp_path / "dds_scene.gltf"
    w.write_gltf(path)
    return path


def test_host_mirror_native_route(pkg, tmp_path):
    rng = np.random.default_rng(3)
    # unique extents name the textures: BC1 colour + BC3 normal map, BC5 colour + BC1 normal map, BC3 colour
    texs = [_bc(rng, 8, 8, BC1_SRGB), _bc(rng, 16, 8, BC3_SRGB, levels=1), _bc(rng, 12, 20, BC5_UNORM), _bc(rng, 4, 16, BC1_UNORM),
            _bc(rng, 20, 12, BC3_SRGB)]
    colour = (0, 2, 4)
    # the BC3 colour texture starts with a block of alpha 0 over a colour: PremultiplyTextureData would zero it
    texs[4].data[:16] = np.frombuffer(bytes(8) + struct.pack("<HHI", 0xFFFF, 0x8410, 0), np.uint8)
    first = bc_ref.decode_level(texs[4].data[:16 * 15], 20, 12, BC3_SRGB)[0, 0]
    assert first.tolist() == [255, 255, 255, 0]
    file = [bc_ref.dds_file(t.data, t.w, t.h, t.levels, t.fmt) for t in texs]
    path = _dds_scene(tmp_path, [(file[0], file[1]), (file[2], file[3]), (file[4], None)])

    def table(scene):
        return {(t.width, t.height): t for t in _textures(pkg, scene.desc)}

    def opaque(scene):
        d = scene.desc
        return np.frombuffer((C.c_uint8 * (d.geometryCount * 20)).from_address(d.geometries), np.uint8).reshape(-1, 20)[:, 16].tolist()

    native = pkg.Scene("file:" + str(path), native_bc=True)
    got = table(native)
    # TextureUploader::GetImageFormat in full: BC3 always sRGB (a normal map too), BC5 always UNORM (a colour texture too), BC1 by type
    assert [got[(t.w, t.h)].format for t in texs] == [BC1_SRGB, BC3_SRGB, BC5_UNORM, BC1_UNORM, BC3_SRGB]
    for t in texs:
        rec = got[(t.w, t.h)]
        assert rec.levels == t.levels
        blocks = np.frombuffer((C.c_uint8 * len(t.data)).from_address(rec.data), np.uint8)
        assert (blocks == t.data).all()  # the file's blocks as they are: nothing decoded, nothing premultiplied
    assert opaque(native) == [0, 0, 0]  # hasTransparency = true for every .dds, the two-channel BC5 included
    # the same through a description's key
    js = '{"components": ["%s"], "nativeBlockCompression": true}' % str(path)
    described = pkg.Scene("description:" + js)  # (kept alive: the desc points into it)
    assert {k: v.format for k, v in table(described).items()} == {k: v.format for k, v in got.items()}
    # switch off: today's RGBA8 decode, byte for byte -- by type, channel-count transparency, alpha-0 colour texels zeroed
    js = '{"components": ["%s"], "nativeBlockCompression": false}' % str(path)
    for plain in (pkg.Scene("file:" + str(path)), pkg.Scene("file:" + str(path), native_bc=False), pkg.Scene("description:" + js)):
        old = table(plain)
        for k, (t, fmt) in enumerate(zip(texs, (RGBA8_SRGB, RGBA8_UNORM, RGBA8_SRGB, RGBA8_UNORM, RGBA8_SRGB))):
            rec = old[(t.w, t.h)]
            want = bc_ref.twin_texels(t.data, t.w, t.h, t.levels, t.fmt).reshape(-1, 4).copy()
            if k in colour and t.fmt != BC5_UNORM:
                want[want[:, 3] == 0, :3] = 0
            assert rec.format == fmt and rec.levels == t.levels
            assert (np.frombuffer((C.c_uint8 * want.size).from_address(rec.data), np.uint8) == want.reshape(-1)).all()
        assert opaque(plain) == [0, 1, 0]  # BC1 and BC3 have four channels, BC5 two
    assert pkg.load_host().pth_scene_create_ex(b"default", 1.0, 0, 2) is None  # unknown flag bits


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
SHAPES = ((4, 4), (5, 3), (8, 8), (64, 64), (67, 45), (256, 4), (4, 256), (1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_lookups_match_the_twin_bitexact(pkg, orc, gpu_renderer, fmt):
    s = pkg.Scene("texture_test")
    rng = np.random.default_rng(40 + fmt)
    texs = [_bc(rng, w, h, fmt, crafted=(w, h) in ((64, 64), (8, 8), (4, 4))) for w, h in SHAPES]
    d, keep = _desc(pkg, s.desc, texs)
    td, tkeep = _desc(pkg, s.desc, [t.twin() for t in texs])
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == []
    osc = orc.OracleScene(td, build_bvh=False)
    inp = _lookups(50 + fmt, 20000, 9, 9 + len(texs))
    for implicit in (False, True):
        a, b = gpu_renderer.test_texture(inp, implicit), osc.test_texture(inp, implicit)
        assert (a == b).all(), f"{int((a != b).any(axis=1).sum())} samples differ (format {fmt}, implicit {implicit})"


@pytest.mark.gpu
def test_one_level_images(pkg, orc, gpu_renderer):
    """levels = 1 stays a one-level image.  The twin (RGBA8, levels = 1) gets a generated chain, so the two agree wherever both
    sample level 0: implicit LOD, and explicit gradients no longer than one texel.  Beyond that the one-level image can only
    return values inside level 0's range; 1e-6 of slack for the rounding of the bilinear weights and the tap average."""
    s = pkg.Scene("texture_test")
    rng = np.random.default_rng(60)
    texs = [_bc(rng, w, h, fmt, levels=1) for fmt in (BC1_SRGB, BC3_SRGB, BC5_UNORM) for w, h in ((67, 45), (64, 64))]
    d, keep = _desc(pkg, s.desc, texs)
    td, tkeep = _desc(pkg, s.desc, [t.twin() for t in texs])
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == []
    osc = orc.OracleScene(td, build_bvh=False)
    n = 6000
    which = rng.integers(0, len(texs), n)
    wh = np.float32([(texs[k].w, texs[k].h) for k in which])
    uv = rng.uniform(-1.5, 2.5, (n, 2)).astype(np.float32)
    # two gradient vectors of length <= 1 texel each: (dudx w, dvdx h) and (dudy w, dvdy h)
    ang, length = rng.uniform(0, 2 * np.pi, (n, 2)), rng.uniform(0, 0.999, (n, 2))
    gx = np.stack([length[:, 0] * np.cos(ang[:, 0]) / wh[:, 0], length[:, 0] * np.sin(ang[:, 0]) / wh[:, 1]], 1).astype(np.float32)
    gy = np.stack([length[:, 1] * np.cos(ang[:, 1]) / wh[:, 0], length[:, 1] * np.sin(ang[:, 1]) / wh[:, 1]], 1).astype(np.float32)
    small = _inputs(9 + which, uv[:, 0], uv[:, 1], gx[:, 0], gx[:, 1], gy[:, 0], gy[:, 1])
    assert (gpu_renderer.test_texture(small, True) == osc.test_texture(small, True)).all()
    assert (gpu_renderer.test_texture(small, False) == osc.test_texture(small, False)).all()
    big = small.copy()
    big[:, 3:] *= (10.0 ** rng.uniform(0.5, 2.5, (n, 1))).astype(np.float32)
    out = gpu_renderer.test_texture(big, False).view(np.float32)
    for k, t in enumerate(texs):
        px = bc_ref.decode_level(t.data, t.w, t.h, t.fmt).reshape(-1, 4).astype(np.float64) / 255.0
        if bc_ref.TWIN_FORMAT[t.fmt] == RGBA8_SRGB:
            px[:, :3] = np.where(px[:, :3] <= 0.04045, px[:, :3] / 12.92, ((px[:, :3] + 0.055) / 1.055) ** 2.4)
        got = out[which == k]
        assert len(got) > 100 and (got >= px.min(0) - 1e-6).all() and (got <= px.max(0) + 1e-6).all()


@pytest.mark.gpu
def test_upload_rules(pkg, orc, gpu_renderer):
    s = pkg.Scene("texture_test")
    rng = np.random.default_rng(70)
    rgba = _Tex(64, 64, RGBA8_SRGB, 1, rng.integers(0, 256, 64 * 64 * 4, dtype=np.uint8))
    texs = [_bc(rng, 64, 64, BC1_SRGB), _bc(rng, 64, 64, BC3_SRGB), rgba, _bc(rng, 128, 128, BC1_UNORM),
            _bc(rng, 128, 128, BC1_SRGB, levels=1), _bc(rng, 64, 64, BC5_UNORM, levels=3)]
    inp = _lookups(71, 20000, 9, 15)
    idx = inp.view(np.uint32)[:, 0]

    def check(osc, where, what):
        for implicit in (False, True):
            a, b = gpu_renderer.test_texture(inp, implicit), osc.test_texture(inp, implicit)
            assert (a[where] == b[where]).all(), what

    # the 6,000-byte share: the BC textures keep 64 x 64, the RGBA8 one beside them becomes 32 x 32
    d, keep = _desc(pkg, s.desc, texs, budget=6 * SHARE)
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == [4, 5]  # 128 x 128 with one level; 64 x 64 with 3 of its 7 levels
    # ... as the twins at an unlimited budget: the 128 x 128 chain is its file levels 1 - 7, the rejected ones are the white texel
    twins = [texs[0].twin(), texs[1].twin(), rgba, texs[3].twin(first=1), _white(), _white()]
    assert (twins[3].w, twins[3].h, twins[3].levels) == (64, 64, 7)
    td, tkeep = _desc(pkg, s.desc, twins)
    unlimited = orc.OracleScene(td, build_bvh=False)
    check(unlimited, idx != 11, "BC textures at the 6,000-byte share")
    rejected = gpu_renderer.test_texture(inp, False).view(np.float32)[(idx == 13) | (idx == 14)]
    assert len(rejected) > 1000 and (rejected == 1.0).all()
    td2, tkeep2 = _desc(pkg, s.desc, twins, budget=6 * SHARE)
    squeezed = orc.OracleScene(td2, build_bvh=False)
    check(squeezed, idx == 11, "the RGBA8 texture at the 6,000-byte share")
    a, b = gpu_renderer.test_texture(inp, True), unlimited.test_texture(inp, True)
    assert (a[idx == 11] != b[idx == 11]).any()  # (it was squeezed)
    # forceFullTextureSize: everything at its own extent; the incomplete chain stays rejected, at scale 1 it is rejected by rule
    d, keep3 = _desc(pkg, s.desc, texs, budget=6 * SHARE, force_full=True)
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == [5]
    td, tkeep3 = _desc(pkg, s.desc, [texs[0].twin(), texs[1].twin(), rgba, texs[3].twin(), _white(), _white()])
    check(orc.OracleScene(td, build_bvh=False), (idx != 13), "forceFullTextureSize")
    one = inp[idx == 13].copy()
    td, tkeep4 = _desc(pkg, s.desc, [_white()] * 4 + [texs[4].twin(), _white()])
    assert (gpu_renderer.test_texture(one, True) == orc.OracleScene(td, build_bvh=False).test_texture(one, True)).all()

    # A level `skip` of another extent.  The share that asks for scale 2 cannot produce one (w / 2 == w >> 1 for every w), so the
    # case takes the smallest scale that can: at a 2,000-byte share BC1 keeps 32 x 32 (chain of 32: 696 B, of 64: 2,744 B), a
    # 96 x 96 file is scaled by 3 to 32 x 32 with skip = 7 - 6 = 1, and its level 1 is 48 x 48.
    t96 = _bc(rng, 96, 96, BC1_SRGB)
    assert t96.levels == 7 and bc_ref.max_extent(BC1_SRGB, 2000) == 32
    d, keep5 = _desc(pkg, s.desc, [t96] + [_white()] * 5, budget=6 * 2000)
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == [0]
    first = inp.copy()
    first.view(np.uint32)[:, 0] = 9
    assert (gpu_renderer.test_texture(first, False).view(np.float32) == 1.0).all()
    d, keep6 = _desc(pkg, s.desc, [t96] + [_white()] * 5, budget=6 * 2000, force_full=True)
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == []
    td, tkeep6 = _desc(pkg, s.desc, [t96.twin()] + [_white()] * 5)
    osc = orc.OracleScene(td, build_bvh=False)
    assert (gpu_renderer.test_texture(first, False) == osc.test_texture(first, False)).all()

    # a BC skybox is refused, and the handle keeps its scene
    sky = (pkg.TextureDesc * 1)(t96.desc(pkg))
    d.skybox, d.skyboxKind = C.addressof(sky), 1
    with pytest.raises(pkg.PtxError) as e:
        gpu_renderer.upload(d)
    assert _status(e) == 1 and "block-compressed" in str(e.value)
    assert (gpu_renderer.test_texture(first, False) == osc.test_texture(first, False)).all()


def _bc_scene(pkg, name, rng, w, h):
    """`name` with every scene texture replaced by a random-block BC texture with a full chain: colour-like ones BC1_SRGB and
    BC3_SRGB in turn, the others BC5_UNORM and BC1_UNORM in turn.  Returns (scene, desc, twin desc, textures, keep)."""
    s = pkg.Scene(name)
    texs, turn = [], [0, 0]
    for t in _textures(pkg, s.desc):
        colour = t.format == RGBA8_SRGB
        fmt = ((BC1_SRGB, BC3_SRGB) if colour else (BC5_UNORM, BC1_UNORM))[turn[colour] % 2]
        turn[colour] += 1
        texs.append(_bc(rng, w, h, fmt, crafted=len(texs) == 0))
    d, keep = _desc(pkg, s.desc, texs)
    td, tkeep = _desc(pkg, s.desc, [t.twin() for t in texs])
    return s, d, td, texs, (keep, tkeep)


def _render(pkg, r, s, W, H, depth, spp, backend):
    r.set_backend(backend)
    try:
        r.resize(W, H)
        r.reset()
        r.render(s.uniform(W, H, bounces=depth, sample_count=spp), s.lights)
        return r.readback()
    finally:
        r.set_backend(pkg.BACKEND_WAVEFRONT)


@pytest.mark.gpu
@pytest.mark.parametrize("name,extent", (("texture_test", (96, 64)), ("alpha_test", (52, 36))))
def test_frames_match_the_twin_bitexact(pkg, orc, gpu_renderer, name, extent):
    """Through the path, on both backends: texture_test with all three formats; alpha_test with a BC1 punch-through and a BC3
    random-alpha colour texture on its non-opaque geometry (any-hit stages, decal and shadow rule read the decoded pool)."""
    s, d, td, texs, keep = _bc_scene(pkg, name, np.random.default_rng(80), *extent)
    assert {t.fmt for t in texs} >= ({BC1_SRGB, BC3_SRGB, BC5_UNORM} if name == "texture_test" else {BC1_SRGB, BC3_SRGB})
    W, H = 96, 64
    ref, _ = orc.OracleScene(td).render(s.uniform(W, H, bounces=3, sample_count=2), s.lights, W, H)
    assert np.isfinite(ref).all() and ref[..., :3].std() > 0
    gpu_renderer.upload(d)
    assert gpu_renderer.textures_rejected() == []
    for backend in (pkg.BACKEND_WAVEFRONT, pkg.BACKEND_MEGAKERNEL):
        img = _render(pkg, gpu_renderer, s, W, H, 3, 2, backend)
        assert _same(img, ref), f"{name}, backend {backend}: {int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())} pixels differ"


@pytest.mark.gpu
def test_streamed_bc_textures(pkg, orc):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    s, d, td, texs, keep = _bc_scene(pkg, "alpha_test", np.random.default_rng(90), 52, 36)
    n = len(texs)
    stand_in = _stand_ins_by_type(s.desc)
    pending, pkeep = _with_textures(pkg, d, [t.desc(pkg, data=False) for t in texs])
    inp = _lookups(91, 6000, 9, 9 + n)
    W, H = 64, 48
    u = s.uniform(W, H, bounces=3, sample_count=2)

    def oracle(desc):
        o = orc.OracleScene(desc)
        return o, o.render(u, s.lights, W, H)[0]

    def frame(r):
        r.resize(W, H)
        r.reset()
        r.render(u, s.lights)
        return r.readback()

    def state(resident):
        """The twin description with every texture outside `resident` behind its stand-in."""
        sd, k = _stand_in_desc(pkg, td, set(range(n)) - set(resident), stand_in)
        return sd, k

    r, b = pkg.Renderer(device=0), pkg.Renderer(device=0)
    try:
        # every texture pending: the oracle of the stand-in scene
        r.upload_streamed(pending, stand_in)
        assert r.texture_residency() == (0, n) and r.textures_rejected() == []
        sd, k0 = state([])
        o, ref = oracle(sd)
        assert (r.test_texture(inp, False) == o.test_texture(inp, False)).all() and _same(frame(r), ref)
        # a partial commit after the build: the alpha re-run
        r.upload_texture(0, texs[0].desc(pkg))
        r.upload_texture(2, texs[2].desc(pkg))
        assert r.commit_textures() == 2 and r.texture_residency() == (2, n - 2)
        sd, k1 = state([0, 2])
        o, ref = oracle(sd)
        assert (r.test_texture(inp, True) == o.test_texture(inp, True)).all() and _same(frame(r), ref)
        # a borrower sees the commit
        b.share_scene(r)
        assert _same(frame(b), ref) and b.textures_rejected() == []
        # the rest: streamed == blocking == the twin's oracle
        with pytest.raises(pkg.PtxError) as e:
            r.upload_texture(0, texs[0].desc(pkg))
        assert _status(e) == 1
        for i in range(n):
            if i not in (0, 2):
                r.upload_texture(i, texs[i].desc(pkg))
        assert r.commit_textures() == n - 2 and r.texture_residency() == (n, 0)
        o, ref = oracle(td)
        streamed = frame(r)
        assert (r.test_texture(inp, False) == o.test_texture(inp, False)).all() and _same(streamed, ref) and _same(frame(b), ref)
        b.close()
        # commit BEFORE the build picks the tables up too
        r.upload_streamed(pending, stand_in, build=False)
        for i in range(n):
            r.upload_texture(i, texs[i].desc(pkg))
        assert r.commit_textures() == n
        r._check(r.lib.ptx_build_accel(r.handle))
        assert _same(frame(r), ref)
        r.upload(d)
        assert _same(frame(r), ref)

        # a rejected texture is resident at once, is never pending, and its upload is refused
        lone = _bc(np.random.default_rng(92), 128, 128, BC1_SRGB, levels=1)
        mixed = [lone] + texs[1:]
        md, mk = _with_textures(pkg, d, [t.desc(pkg, data=False) for t in mixed], budget=n * SHARE)
        r.upload_streamed(md, stand_in)
        assert r.textures_rejected() == [0] and r.texture_residency() == (1, n - 1)
        with pytest.raises(pkg.PtxError) as e:
            r.upload_texture(0, lone.desc(pkg))
        assert _status(e) == 1 and "rejected" in str(e.value)
        out = r.test_texture(inp[inp.view(np.uint32)[:, 0] == 9], False).view(np.float32)
        assert len(out) and (out == 1.0).all()
    finally:
        b.close()
        r.close()


@pytest.mark.gpu
def test_scene_without_bc_textures_is_untouched(pkg, orc, gpu_renderer):
    s = pkg.Scene("texture_test")
    gpu_renderer.upload(s)
    assert gpu_renderer.textures_rejected() == []
    assert gpu_renderer.lib.ptx_textures_rejected(gpu_renderer.handle, None, 0) == 0
    inp = _lookups(95, 20000, 9, 17)
    osc = orc.OracleScene(s.desc, build_bvh=False)
    for implicit in (False, True):
        assert (gpu_renderer.test_texture(inp, implicit) == osc.test_texture(inp, implicit)).all()
