"""Helpers shared by the tests."""
import ctypes as C
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def open_golden(name):
    """A golden-vector file (text mode): they are committed gzip-compressed (decimal uint32 bit patterns compress 4x)."""
    import gzip

    return gzip.open(os.path.join(GOLDEN_DIR, name + ".gz"), "rt")

GEOMETRY_DT = np.dtype([("VertexOffset", "u4"), ("VertexLength", "u4"), ("IndexOffset", "u4"), ("IndexLength", "u4"),
                        ("IsOpaque", "u1"), ("IsAnimated", "u1"), ("pad", "u1", 2)])
MESH_DT = np.dtype([("GeometryIndex", "u4"), ("MaterialId", "u4"), ("TransformIndex", "u4")])
MODEL_DT = np.dtype([("MeshOffset", "u4"), ("MeshCount", "u4")])
INSTANCE_DT = np.dtype([("ModelIndex", "u4"), ("Transform", "f4", 12)])


def _view(ptr, count, dtype):
    if not ptr or not count:
        return np.zeros(0, dtype)
    buf = (C.c_uint8 * (count * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=count)


def desc_arrays(desc):
    return {
        "vertices": _view(desc.vertices, desc.vertexCount * 14, np.dtype("f4")).reshape(-1, 14),
        "indices": _view(desc.indices, desc.indexCount, np.dtype("u4")),
        "transforms": _view(desc.transforms, desc.transformCount * 12, np.dtype("f4")).reshape(-1, 12),
        "geometries": _view(desc.geometries, desc.geometryCount, GEOMETRY_DT),
        "meshes": _view(desc.meshes, desc.meshCount, MESH_DT),
        "models": _view(desc.models, desc.modelCount, MODEL_DT),
        "instances": _view(desc.instances, desc.instanceCount, INSTANCE_DT),
    }


def pair_first(desc):
    """First global triangle id of every (instance, mesh) pair, in instance-then-mesh order --
    the numbering both the oracle (global id) and the HIP path ((pair, prim)) use."""
    a = desc_arrays(desc)
    first, tri = [], 0
    for inst in a["instances"]:
        m = a["models"][inst["ModelIndex"]]
        for k in range(m["MeshCount"]):
            rec = a["meshes"][m["MeshOffset"] + k]
            first.append(tri)
            tri += int(a["geometries"][rec["GeometryIndex"]]["IndexLength"]) // 3
    first.append(tri)
    return np.array(first, dtype=np.int64)


def load_golden(mode):
    with open_golden(f"golden_{mode}.json") as f:
        g = json.load(f)
    out = {}
    for name, c in g.items():
        out[name] = (c["fn"], np.array(c["in"], dtype=np.uint32).reshape(-1, c["nin"]),
                     np.array(c["out"], dtype=np.uint32).reshape(-1, c["nout"]))
    return out


def bits_equal_or_both_nan(a_u32, b_u32):
    af, bf = a_u32.view(np.float32), b_u32.view(np.float32)
    return (a_u32 == b_u32) | (np.isnan(af) & np.isnan(bf))


def ulp_error(got, truth):
    """|got - truth| in units of the binary32 spacing at `truth` (a float64 array): 2^(e - 23) for 2^e <= |truth| < 2^(e + 1),
    and the denormal spacing 2^-149 everywhere below 2^-126.  For finite `truth` inside the binary32 range."""
    truth = np.asarray(truth, np.float64)
    _, e = np.frexp(truth)  # |truth| = m * 2^e with m in [0.5, 1)
    spacing = np.ldexp(1.0, np.maximum(e - 1, -126) - 23)
    return np.abs(np.asarray(got, np.float64) - truth) / spacing


def half_ordinal(x):
    """The position of every value of `x` (binary16-valued floats, infinities included) on the binary16 number line: the sign
    times the magnitude's bit pattern, so neighbouring binary16 values differ by one and +-0 are both 0."""
    h = np.asarray(x).astype(np.float16).view(np.uint16).astype(np.int64)
    return np.where(h & 0x8000, -(h & 0x7fff), h & 0x7fff)


def rel_l2(img, ref):
    return float(np.linalg.norm((img[..., :3] - ref[..., :3]).astype(np.float64)) /
                 max(np.linalg.norm(ref[..., :3].astype(np.float64)), 1e-30))


def random_rays(rng, n, lo, hi, tmax=1e4):
    """Rays with origins in the box [lo,hi] pointing in random directions (float32, 8 per ray)."""
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = 1e-5
    rays[:, 4:7] = d
    rays[:, 7] = tmax
    return rays


# ---------------------------------------------------------------------------------------
# the tile-shard message of the gather (include/ptx.h: PtxTileShard, ptx_pack_shard, ptx_unpack_shards)
# ---------------------------------------------------------------------------------------
def pack_shard(img, mask_tiles, tile, W, H):
    """Dense tile-major shard buffer [ownedTile][tile*tile][4] in the slot order of
    csrc/pt_wavefront.hpp slotPixel(): 8x8 pixel blocks inside a tile."""
    tiles_x = (W + tile - 1) // tile
    out = np.zeros((len(mask_tiles), tile * tile, 4), np.float32)
    bpr = tile // 8
    o = np.arange(tile * tile)
    blk, ib = o // 64, o % 64
    lx, ly = (blk % bpr) * 8 + ib % 8, (blk // bpr) * 8 + ib // 8
    for k, t in enumerate(mask_tiles):
        x, y = (t % tiles_x) * tile + lx, (t // tiles_x) * tile + ly
        ok = (x < W) & (y < H)
        out[k, ok] = img[y[ok], x[ok]]
    return out


def unpack_shard(buf, mask_tiles, tile, W, H, img):
    tiles_x = (W + tile - 1) // tile
    bpr = tile // 8
    o = np.arange(tile * tile)
    blk, ib = o // 64, o % 64
    lx, ly = (blk % bpr) * 8 + ib % 8, (blk // bpr) * 8 + ib // 8
    for k, t in enumerate(mask_tiles):
        x, y = (t % tiles_x) * tile + lx, (t // tiles_x) * tile + ly
        ok = (x < W) & (y < H)
        img[y[ok], x[ok]] = buf[k, ok]


def shard_entries(W, H, rank, world, tile):
    """The message of one rank, entry by entry, as include/ptx.h words it: the image is cut into tile x tile tiles numbered
    row-major; the rank owns the tiles with tile % world == rank and its message holds them in increasing order, tile * tile
    entries each; inside a tile the entries run over 8x8 pixel blocks in row-major order, inside a block over its pixels in
    row-major order.  Returns int64[ownedTiles * tile * tile]: the row-major pixel index (y * W + x) of every entry, -1 for the
    entries of a ragged tile that lie outside the image."""
    assert tile >= 8 and tile % 8 == 0 and 0 <= rank < world
    tiles_x, tiles_y = -(-W // tile), -(-H // tile)
    blocks_per_row = tile // 8
    out = []
    for t in range(tiles_x * tiles_y):
        if t % world != rank:
            continue
        x0, y0 = (t % tiles_x) * tile, (t // tiles_x) * tile
        e = np.arange(tile * tile, dtype=np.int64)
        block, inside = e // 64, e % 64
        x = x0 + (block % blocks_per_row) * 8 + inside % 8
        y = y0 + (block // blocks_per_row) * 8 + inside // 8
        out.append(np.where((x < W) & (y < H), y * W + x, -1))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def gather_index(W, H, world, tile, stride_entries):
    """For every pixel (row-major) the entry of the gather's receive buffer it comes from: the pieces of ranks 0 .. world-1 lie
    `stride_entries` entries apart.  Written per pixel (which tile, whose, the how-manyeth of that rank, which 8x8 block of the
    tile, which pixel of the block), not by inverting shard_entries.  Returns int64[W * H]."""
    assert tile >= 8 and tile % 8 == 0
    tiles_x = -(-W // tile)
    y, x = np.divmod(np.arange(W * H, dtype=np.int64), W)
    t = (y // tile) * tiles_x + x // tile
    rank, nth = t % world, t // world
    lx, ly = x % tile, y % tile
    block = (ly // 8) * (tile // 8) + lx // 8
    return rank * stride_entries + nth * tile * tile + block * 64 + (ly % 8) * 8 + lx % 8


# (W, H, world, tile) -> (tiles_x, tiles_y, fewest owned tiles, most, empty ranks, entries outside the image), why the case is here
SHARD_CASES = {
    (1920, 1080, 4, 32): (60, 34, 510, 510, 0, 15360),   # BASELINE configs[3]
    (1920, 1080, 8, 32): (60, 34, 255, 255, 0, 15360),   # the strong-scaling frame: equal tiles, unequal pixels per rank
    (3840, 2160, 8, 32): (120, 68, 1020, 1020, 0, 61440),  # configs[4], bench.py's default tile
    (3840, 2160, 8, 16): (240, 135, 4050, 4050, 0, 0),   # configs[4] as test_long_sample_schedules shards it
    (512, 512, 8, 32): (16, 16, 32, 32, 0, 0),           # configs[0]; tiles_x % world == 0: a rank owns whole columns
    (200, 120, 3, 32): (7, 4, 9, 10, 0, 4672),           # unequal shards
    (328, 200, 2, 32): (11, 7, 38, 39, 0, 13248),        # the bench test's shape
    (328, 200, 5, 8): (41, 25, 205, 205, 0, 0),          # smallest tile: one block per tile row
    (328, 200, 7, 64): (6, 4, 3, 4, 0, 32704),           # large tile, prime world, 5,120 pixels beside 12,800
    (257, 33, 5, 24): (11, 2, 4, 5, 0, 4191),            # 3 blocks per tile row
    (131, 77, 1, 40): (4, 2, 8, 8, 0, 2713),             # 5 blocks per tile row; world 1 through the gather
    (33, 257, 6, 16): (3, 17, 8, 9, 0, 4575),            # tall image, a rank with 128 pixels
    (640, 360, 8, 128): (5, 3, 1, 2, 0, 15360),          # one and two owned tiles
    (96, 54, 8, 32): (3, 2, 0, 1, 2, 960),               # more ranks than tiles
    (100, 70, 16, 32): (4, 3, 0, 1, 4, 5288),            # world 16
    (7, 5, 3, 8): (1, 1, 0, 1, 2, 29),                   # image smaller than a tile
    (1, 1, 2, 8): (1, 1, 0, 1, 1, 63),
}
SHARD_SENTINEL = 0x7FC5A5A5  # a quiet NaN with a recognisable payload: what no renderer writes


def render_pair(pkg, orc, name, detail, W, H, frames, depth, backend=0, brute=False, lens=0.0, sample_count=1, tile=None):
    """Render `frames` launches with the HIP path and with the oracle; returns both accumulation images
    after checking that segment / shadow-ray / sample / retry counts agree launch by launch."""
    scene = pkg.Scene(name, detail)
    lights = scene.lights
    r = pkg.Renderer(backend=backend)
    r.upload(scene)
    r.resize(W, H)
    if tile:
        r.set_tile_shard(0, 1, tile)
    osc = orc.OracleScene(scene.desc, build_bvh=not brute)
    ref = np.zeros((H, W, 4), np.float32)
    seg = shadow = 0
    for f in range(frames):
        u = scene.uniform(W, H, bounces=depth, sample_count=sample_count, total_samples=f * sample_count, lens_radius=lens, focal_distance=6.0)
        r.render(u, lights)
        st = r.stats()
        _, ost = osc.render(u, lights, W, H, accum=ref, brute_force=brute)
        assert st.segments == ost.segments and st.shadowRays == ost.shadowRays, "segment counts differ"
        assert st.pathSamples == ost.pathSamples and st.retries == ost.retries
        seg += st.segments
        shadow += st.shadowRays
    img = r.readback()
    r.close()
    return img, ref


def known_answer_rays():
    """Rays found by tools/full_size_sweep.py on which a tree walk once disagreed with brute force:
    (scene, origin bits, direction bits).  street_like: rays crossing a triangle next to an edge, 12 - 40 units from the
    camera, where plain Moeller-Trumbore also accepted the neighbouring triangle (equal t, smaller id) although the point
    lay outside its box; atrium_like: a zero-area triangle (e1 == e2) that the triangle test used to "hit" at a
    meaningless t."""
    return [
        ("street_like", (0xC2080000, 0x3FD9999C, 0x3F800000), (0x3F4C1984, 0xBD9D0A84, 0xBF194709)),
        ("street_like", (0xC2080000, 0x3FD9999C, 0x3F800000), (0x3F7DA424, 0x3C974EA6, 0x3E09645E)),
        ("street_like", (0xC2080000, 0x3FD9999C, 0x3F800000), (0x3F7CF07B, 0xBCDD1A10, 0x3E1B6E52)),
        ("atrium_like", (0xC1880001, 0x3FE66663, 0xBF4CCCCD), (0x3F741F4C, 0x3E64162A, 0x3E4F6AC2)),
    ]


def known_answer_ray_array(scene_name):
    rays = []
    for name, o, d in known_answer_rays():
        if name == scene_name:
            ob, db = np.array(o, np.uint32).view(np.float32), np.array(d, np.uint32).view(np.float32)
            rays.append([ob[0], ob[1], ob[2], 1e-5, db[0], db[1], db[2], 1e4])
    return np.array(rays, np.float32)


def reciprocal_inputs():
    """Bit patterns for the specified reciprocal (PTX_FN_DIVIDE): all 2^23 mantissas of [1, 2) with both signs (the Newton step is
    exact-scaling invariant inside the normal range), every exponent with 4,096 mantissas each (the flush boundaries 2^-126 and
    2^126 lie in there), zero, denormals, infinities, NaNs and the patterns either side of both boundaries."""
    m = np.arange(1 << 23, dtype=np.uint32)
    parts = [np.uint32(0x3f800000) | m, np.uint32(0xbf800000) | m]
    rng = np.random.default_rng(11)
    mant = np.concatenate([np.uint32([0, 1, 0x7fffff, 0x7ffffe, 0x400000]), rng.integers(0, 1 << 23, 4091, dtype=np.uint32)])
    for e in range(256):
        parts.append((np.uint32(e << 23) | mant))
        parts.append((np.uint32(0x80000000 | (e << 23)) | mant))
    parts.append(np.uint32([0, 0x80000000, 1, 0x007fffff, 0x00800000, 0x00800001, 0x7e800000, 0x7e800001, 0x7e7fffff, 0x7f7fffff, 0x7f800000,
                            0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001]))
    return np.concatenate(parts)


def reciprocal_spec(b):
    """The definition (oracle/pt_oracle_math.h pto_rcp) in numpy: RN(1 / b) on [2^-126, 2^126], +-inf below, +-0 above."""
    b = b.astype(np.float32)
    with np.errstate(all="ignore"):
        r = (np.float32(1.0) / b).astype(np.float32)
        ab = np.abs(b)
        r = np.where(ab < np.float32(1.17549435e-38), np.copysign(np.float32(np.inf), b), r)
        r = np.where(ab > np.float32(8.50705917e37), np.copysign(np.float32(0.0), b), r)
        r = np.where(np.isnan(b), b, r)
    return r.astype(np.float32)


# ---------------------------------------------------------------------------------------
# hand-built scenes and the closest-hit comparisons that use them
# ---------------------------------------------------------------------------------------
IDENTITY_3X4 = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


def mr_material(color=(1, 1, 1), roughness=1.0, metalness=0.0, ior=1.5, transmission=0.0, att_color=(1, 1, 1), att_dist=1e32):
    """One metallic-roughness material record (24 words) with the default texels."""
    m = np.zeros(24, np.float32)
    m[4:8] = (*color, 1.0)
    m[8], m[9], m[10], m[11] = roughness, metalness, ior, transmission
    m[12:15] = att_color
    m[15] = att_dist
    m.view(np.uint32)[19:24] = (4, 0, 1, 2, 3)  # default emissive / colour / normal / roughness / metallic texels
    return m


def quad_mesh(corners, normal):
    """A planar quad as a mesh of two triangles (0 1 2, 2 3 0) over four shared vertices, with the given normal and the
    tangent frame of its first edge."""
    corners = np.asarray(corners, np.float32)
    n = np.asarray(normal, np.float32)
    assert np.cross(corners[1] - corners[0], corners[2] - corners[0]) @ n > 0, "winding must agree with the normal"
    return {"positions": corners, "indices": np.uint32([0, 1, 2, 2, 3, 0]), "normal": n,
            "uv": np.float32([[k in (1, 2), k in (2, 3)] for k in range(4)])}


def _mesh_vertices(mesh):
    """Rows of 14 floats (position, uv, normal, tangent, bitangent) and the index list of one mesh: a dict from quad_mesh
    or an (n, 3, 3) array of triangles (own vertices each, the geometric normal; +z / +x for a zero-area triangle)."""
    if isinstance(mesh, dict):
        p, idx = np.asarray(mesh["positions"], np.float32), np.asarray(mesh["indices"], np.uint32)
        n = np.broadcast_to(np.asarray(mesh["normal"], np.float32), p.shape)
        t = p[1] - p[0]
        t = np.broadcast_to(t / np.linalg.norm(t), p.shape)
        uv = np.asarray(mesh["uv"], np.float32)
    else:
        tri = np.asarray(mesh, np.float32).reshape(-1, 3, 3)
        p, idx = tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.uint32)
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        nn = np.cross(e1, e2)
        ln, lt = np.linalg.norm(nn, axis=1, keepdims=True), np.linalg.norm(e1, axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            nn = np.where(ln > 0, nn / ln, np.float32([0, 0, 1]))
            tt = np.where((lt > 0) & (ln > 0), e1 / lt, np.float32([1, 0, 0]))
        n, t = np.repeat(nn, 3, axis=0), np.repeat(tt, 3, axis=0)
        uv = np.tile(np.float32([[0, 0], [1, 0], [0, 1]]), (len(tri), 1))
    b = np.cross(n, t)
    return np.concatenate([p, uv, n, t, b], axis=1).astype(np.float32), idx


class TriangleSoup:
    """A PtxSceneDesc assembled from numpy arrays that this object keeps alive: `models` is a list of models, each a list of
    meshes (world-space (n, 3, 3) triangle arrays or quad_mesh dicts); `instances` a list of (model index, 3x4 transform),
    by default one identity instance per model; every mesh uses the one metallic-roughness `material`."""

    def __init__(self, pkg, models, instances=None, material=None):
        verts, inds, geos, meshes, model_rows = [], [], [], [], []
        nv = ni = 0
        for model in models:
            model_rows.append((len(meshes), len(model)))
            for mesh in model:
                v, idx = _mesh_vertices(mesh)
                geos.append((nv, len(v), ni, len(idx), 1, 0, (0, 0)))
                meshes.append((len(geos) - 1, 0, 0))
                verts.append(v)
                inds.append(idx)
                nv, ni = nv + len(v), ni + len(idx)
        if instances is None:
            instances = [(m, IDENTITY_3X4) for m in range(len(models))]
        self.vertices = np.ascontiguousarray(np.concatenate(verts), np.float32)
        self.indices = np.ascontiguousarray(np.concatenate(inds), np.uint32)
        self.transforms = IDENTITY_3X4.reshape(1, 12).copy()
        self.geometries = np.array(geos, GEOMETRY_DT)
        self.materials = np.ascontiguousarray(mr_material() if material is None else material, np.float32).reshape(1, 24)
        self.meshes = np.array(meshes, MESH_DT)
        self.models = np.array(model_rows, MODEL_DT)
        self.instances = np.array([(m, np.asarray(x, np.float32).reshape(12)) for m, x in instances], INSTANCE_DT)
        d = pkg.SceneDesc()
        d.vertices, d.vertexCount = self.vertices.ctypes.data, len(self.vertices)
        d.indices, d.indexCount = self.indices.ctypes.data, len(self.indices)
        d.transforms, d.transformCount = self.transforms.ctypes.data, 1
        d.geometries, d.geometryCount = self.geometries.ctypes.data, len(self.geometries)
        d.metallicRoughnessMaterials, d.metallicRoughnessMaterialCount = self.materials.ctypes.data, 1
        d.meshes, d.meshCount = self.meshes.ctypes.data, len(self.meshes)
        d.models, d.modelCount = self.models.ctypes.data, len(self.models)
        d.instances, d.instanceCount = self.instances.ctypes.data, len(self.instances)
        self.desc = d


def world_triangles(desc, instance_transforms=None):
    """Every triangle of a scene in world space, float64, in the global order (instance, mesh, primitive): (n, 3, 3)."""
    a = desc_arrays(desc)
    tris = []
    for i, inst in enumerate(a["instances"]):
        x = inst["Transform"] if instance_transforms is None else np.asarray(instance_transforms, np.float32).reshape(-1, 12)[i]
        it = np.float64(x).reshape(3, 4)
        m = a["models"][inst["ModelIndex"]]
        for k in range(m["MeshCount"]):
            rec = a["meshes"][m["MeshOffset"] + k]
            g = a["geometries"][rec["GeometryIndex"]]
            mt = np.float64(a["transforms"][rec["TransformIndex"]]).reshape(3, 4)
            M = np.vstack([it, [0, 0, 0, 1]]) @ np.vstack([mt, [0, 0, 0, 1]])
            v = np.float64(a["vertices"][g["VertexOffset"]:g["VertexOffset"] + g["VertexLength"], 0:3])
            idx = a["indices"][g["IndexOffset"]:g["IndexOffset"] + g["IndexLength"]].reshape(-1, 3)
            w = v @ M[:3, :3].T + M[:3, 3]
            tris.append(w[idx])
    return np.concatenate(tris) if tris else np.zeros((0, 3, 3))


def moller_trumbore_f64(T, ray):
    """The textbook Moeller-Trumbore test in float64 of one ray (8 floats) against every triangle of T (n, 3, 3):
    (inside, t, u, v, margin) per triangle, margin = the smallest barycentric (negative outside)."""
    o, dr, tmin, tmax = np.float64(ray[0:3]), np.float64(ray[4:7]), np.float64(ray[3]), np.float64(ray[7])
    v0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    p = np.cross(dr, e2)
    det = np.einsum("ij,ij->i", e1, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v0
        u = np.einsum("ij,ij->i", s, p) * inv
        q = np.cross(s, e1)
        v = (q @ dr) * inv
        t = np.einsum("ij,ij->i", e2, q) * inv
    inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < tmax) & (np.abs(det) > 1e-300)
    margin = np.minimum(np.minimum(u, v), 1 - u - v)
    return inside, t, u, v, margin


def global_ids(desc, ids):
    """(pair, prim) pairs of ptx_trace_rays -> global triangle ids (0xffffffff = miss), the oracle's numbering."""
    first = pair_first(desc)
    miss = ids[:, 0] == 0xFFFFFFFF
    pair = ids[:, 0].astype(np.int64)
    assert (pair[~miss] < len(first) - 1).all(), "a hit names an (instance, mesh) pair the scene does not have"
    prim = ids[:, 1].astype(np.int64)
    assert (prim[~miss] < (first[1:] - first[:-1])[pair[~miss]]).all(), "a hit names a primitive its pair does not have"
    return np.where(miss, 0xFFFFFFFF, first[np.where(miss, 0, pair)] + prim).astype(np.uint32)


def check_trace_against_bruteforce(r, orc, desc, rays, min_hits, instance_transforms=None, label="", bones=None):
    """Closest-hit and occlusion queries of renderer `r` (its tree over `desc`) against the oracle's brute force: the same
    global triangle per ray, t / u / v bit for bit on hits, the same occlusion flag -- and at least `min_hits` hits, so that a
    scene every ray misses cannot pass.  `bones` (m x 12): the oracle skins its animated meshes with them (None: the bind pose).
    Returns the brute-force closest hits."""
    osc = orc.OracleScene(desc, build_bvh=False, instance_transforms=instance_transforms, bones=bones)
    want = osc.trace_closest(rays, brute_force=True)
    occ_want = osc.trace_any(rays, brute_force=True)
    osc.close()
    hits, ids = r.trace_rays(rays, any_hit=False)
    gid = global_ids(desc, ids)
    bad = np.flatnonzero(gid != want["tri"])
    assert not len(bad), f"{label}: {len(bad)} rays hit a different triangle, first ray {bad[0]}: {gid[bad[0]]} != {want['tri'][bad[0]]}"
    h = want["tri"] != 0xFFFFFFFF
    assert int(h.sum()) >= min_hits, f"{label}: only {int(h.sum())} hits"
    for k, f in enumerate(("t", "u", "v")):
        diff = np.flatnonzero(hits[h, k].view(np.uint32) != want[f][h].view(np.uint32))
        assert not len(diff), f"{label}: {f} differs on {len(diff)} hits"
    occ, _ = r.trace_rays(rays, any_hit=True)
    assert ((occ[:, 3] != 0) == (occ_want != 0)).all(), f"{label}: occlusion differs on {int(((occ[:, 3] != 0) != (occ_want != 0)).sum())} rays"
    return want


def check_closest_against_float64(T, rays, got, t_slack=0.0, bary_slack=0.0):
    """Closest hits `got` (the oracle's trace_closest record) against moller_trumbore_f64 over the world-space triangles T:
    hit / miss agrees except where the float64 barycentrics sit within 1e-5 of an edge; the nearest triangle agrees except
    between hits closer than 1e-4 of t; t, u, v agree to float precision.  Far from the origin the float32 arithmetic works on
    coordinates whose ulp is no longer small: t_slack (world units) and bary_slack (barycentric units) widen every bound by
    that much.  Returns (float64 hits, same triangle, other triangle)."""
    hits = agree = close = 0
    for r in range(len(rays)):
        inside, t, u, v, margin = moller_trumbore_f64(T, rays[r])
        if not inside.any():
            # a miss in float64: the oracle may only report a hit that grazes an edge
            if got["tri"][r] != 0xFFFFFFFF:
                k = int(got["tri"][r])
                assert abs(margin[k]) < 1e-5 + bary_slack, (r, margin[k])
            continue
        hits += 1
        tb = np.where(inside, t, np.inf)
        k = int(np.argmin(tb))
        if got["tri"][r] == 0xFFFFFFFF:
            assert margin[k] < 1e-5 + bary_slack, (r, margin[k])   # the only float64 hit grazes an edge
            continue
        kg = int(got["tri"][r])
        if kg == k:
            agree += 1
            assert abs(got["t"][r] - t[k]) <= 2e-5 * max(1.0, t[k]) + t_slack and abs(got["u"][r] - u[k]) < 1e-4 + bary_slack and \
                abs(got["v"][r] - v[k]) < 1e-4 + bary_slack, (r, got[r], t[k], u[k], v[k])
        else:
            # another triangle: it must be a genuine float64 hit at (nearly) the same distance, or an edge case
            close += 1
            assert (inside[kg] and abs(t[kg] - t[k]) < 1e-4 * max(1.0, t[k]) + t_slack) or margin[k] < 1e-5 + bary_slack or \
                abs(margin[kg]) < 1e-5 + bary_slack, (r, t[k], t[kg])
    return hits, agree, close
