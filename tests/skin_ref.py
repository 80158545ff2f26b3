"""Linear-blend skinning from its definition (skinning.comp:21-50) in numpy, generic over the dtype, and a
scene builder for skinned geometry.  Independent of the oracle's skinVertex and of k_skin: matrix operations over all vertices at
once, the inverse from LAPACK.  float32 restates the arithmetic up to evaluation order, float64 is what both approximate; the
tolerances of tests/test_skinning.py are measured between the two.  Never calls the oracle or the HIP library."""
import ctypes as C
import os
import re

import numpy as np

import util

ANIMATED_VERTEX_DT = np.dtype([("Position", "f4", 3), ("TexCoords", "f4", 2), ("Normal", "f4", 3), ("Tangent", "f4", 3), ("Bitangent", "f4", 3),
                               ("BoneIndices", "u4", 4), ("BoneWeights", "f4", 4)])
SCENE_TEXTURE_OFFSET = 9  # PTX_SCENE_TEXTURE_OFFSET: texture i of the scene has shader index 9 + i


def _unit(x):
    with np.errstate(all="ignore"):
        return x / np.sqrt(np.einsum("...i,...i->...", x, x))[..., None]


def skin_vertices(animated, bones, dtype):
    """Rows of 14 values (position, uv, normal, tangent, bitangent) in `dtype` for ANIMATED_VERTEX_DT rows `animated` posed by
    `bones` (m x 12, a 3 x 4 affine matrix each).  Up to four (index, weight) slots count, in order, while the running weight is
    below 1; an index at or above m is the identity; the position goes through the affine matrix, tangent and bitangent through
    its linear part, the normal through the inverse transpose of the linear part, each direction normalised per bone before it
    is weighted; the sums are not normalised; the texture coordinates are copied."""
    a = np.asarray(animated, ANIMATED_VERTEX_DT)
    b = np.asarray(bones, np.float32).reshape(-1, 3, 4).astype(dtype)
    table = np.concatenate([b, np.eye(3, 4, dtype=dtype)[None]])  # the last row stands for every index out of range
    slot = np.minimum(a["BoneIndices"].astype(np.int64), len(b))
    w = a["BoneWeights"].astype(dtype)
    assert (w >= 0).all(), "the running weight must not decrease"
    running = np.cumsum(w, axis=1, dtype=dtype) - w  # the weight taken before each slot
    w = np.where(running < 1, w, dtype(0))
    M = table[slot]  # (n, 4, 3, 4)
    A, t = M[..., 0:3], M[..., 3]
    A_inv_t = np.linalg.inv(A).swapaxes(-1, -2)
    out = np.zeros((len(a), 14), dtype)
    out[:, 0:3] = np.einsum("nk,nki->ni", w, np.einsum("nkij,nj->nki", A, a["Position"].astype(dtype)) + t)
    out[:, 3:5] = a["TexCoords"]
    out[:, 5:8] = np.einsum("nk,nki->ni", w, _unit(np.einsum("nkij,nj->nki", A_inv_t, a["Normal"].astype(dtype))))
    out[:, 8:11] = np.einsum("nk,nki->ni", w, _unit(np.einsum("nkij,nj->nki", A, a["Tangent"].astype(dtype))))
    out[:, 11:14] = np.einsum("nk,nki->ni", w, _unit(np.einsum("nkij,nj->nki", A, a["Bitangent"].astype(dtype))))
    return out


def bind_vertices(animated, dtype):
    """The attributes as authored: what the skinned block holds until the first update."""
    a = np.asarray(animated, ANIMATED_VERTEX_DT)
    return np.concatenate([a["Position"], a["TexCoords"], a["Normal"], a["Tangent"], a["Bitangent"]], axis=1).astype(dtype)


def animated_rows(mesh, indices, weights, classes=None):
    """ANIMATED_VERTEX_DT rows and the index list of one mesh (whatever util._mesh_vertices takes) with per-vertex bone `indices`
    (n, 4) and `weights` (n, 4); `classes` (n) labels the vertices for failure messages."""
    v, idx = util._mesh_vertices(mesh)
    rows = np.zeros(len(v), ANIMATED_VERTEX_DT)
    rows["Position"], rows["TexCoords"], rows["Normal"], rows["Tangent"], rows["Bitangent"] = v[:, 0:3], v[:, 3:5], v[:, 5:8], v[:, 8:11], v[:, 11:14]
    rows["BoneIndices"], rows["BoneWeights"] = indices, weights
    cls = np.full(len(v), -1, np.int64) if classes is None else np.asarray(classes, np.int64)
    return {"animated": rows, "indices": idx, "classes": cls}


def declared_animated_vertex_size(pkg):
    """sizeof(PtxAnimatedVertex) as include/ptx.h declares it: arrays of 4-byte scalars in the scalar block layout."""
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    body = re.search(r"typedef struct PtxAnimatedVertex \{(.*?)\} PtxAnimatedVertex;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t) \w+\[(\d+)\];", body, re.M)
    assert len(fields) == len(ANIMATED_VERTEX_DT.names)
    return sum(4 * int(n) for _, n in fields)


class SkinnedSoup:
    """A PtxSceneDesc of static and animated meshes, assembled from numpy arrays this object keeps alive.  `models`: a list of
    models, each a list of (mesh, transform index); a mesh is what util._mesh_vertices takes (static) or a dict from
    animated_rows (IsAnimated = 1, vertices and indices in the animated arrays).  `instances`: (model index, 3 x 4 transform),
    several per model allowed.  `transforms`: the mesh transforms (row 0 should be the identity).  `normal_texel`: an RGBA32F
    value for one 1 x 1 scene texture that the one metallic-roughness material then uses as its normal map."""

    def __init__(self, pkg, models, instances, transforms=None, material=None, normal_texel=None):
        assert ANIMATED_VERTEX_DT.itemsize == declared_animated_vertex_size(pkg) == 88
        sv, si, av, ai, cls, geos, meshes, model_rows = [], [], [], [], [], [], [], []
        nsv = nsi = nav = nai = 0
        for model in models:
            model_rows.append((len(meshes), len(model)))
            for mesh, transform in model:
                if isinstance(mesh, dict) and "animated" in mesh:
                    rows, idx = mesh["animated"], np.asarray(mesh["indices"], np.uint32)
                    geos.append((nav, len(rows), nai, len(idx), 1, 1, (0, 0)))
                    av.append(rows)
                    ai.append(idx)
                    cls.append(mesh["classes"])
                    nav, nai = nav + len(rows), nai + len(idx)
                else:
                    v, idx = util._mesh_vertices(mesh)
                    geos.append((nsv, len(v), nsi, len(idx), 1, 0, (0, 0)))
                    sv.append(v)
                    si.append(idx)
                    nsv, nsi = nsv + len(v), nsi + len(idx)
                meshes.append((len(geos) - 1, 0, transform))
        cat = lambda parts, dt, shape: np.ascontiguousarray(np.concatenate(parts), dt) if parts else np.zeros(shape, dt)  # noqa: E731
        self.vertices, self.indices = cat(sv, np.float32, (0, 14)), cat(si, np.uint32, 0)
        self.animated_vertices, self.animated_indices = cat(av, ANIMATED_VERTEX_DT, 0), cat(ai, np.uint32, 0)
        self.vertex_class = cat(cls, np.int64, 0)  # per animated vertex
        self.transforms = np.ascontiguousarray(util.IDENTITY_3X4.reshape(1, 12) if transforms is None else transforms, np.float32).reshape(-1, 12)
        self.geometries = np.array(geos, util.GEOMETRY_DT)
        self.materials = np.ascontiguousarray(util.mr_material() if material is None else material, np.float32).reshape(1, 24).copy()
        self.meshes = np.array(meshes, util.MESH_DT)
        self.models = np.array(model_rows, util.MODEL_DT)
        self.instances = np.array([(m, np.asarray(x, np.float32).reshape(12)) for m, x in instances], util.INSTANCE_DT)
        assert (self.meshes["TransformIndex"] < len(self.transforms)).all()
        d = pkg.SceneDesc()
        d.vertices, d.vertexCount = self.vertices.ctypes.data, len(self.vertices)
        d.indices, d.indexCount = self.indices.ctypes.data, len(self.indices)
        d.animatedVertices, d.animatedVertexCount = self.animated_vertices.ctypes.data, len(self.animated_vertices)
        d.animatedIndices, d.animatedIndexCount = self.animated_indices.ctypes.data, len(self.animated_indices)
        d.transforms, d.transformCount = self.transforms.ctypes.data, len(self.transforms)
        d.geometries, d.geometryCount = self.geometries.ctypes.data, len(self.geometries)
        if normal_texel is not None:
            self.texel = np.ascontiguousarray(normal_texel, np.float32).reshape(1, 1, 4)
            self.texture = (pkg.TextureDesc * 1)(pkg.TextureDesc(1, 1, pkg.TEXTURE_RGBA32F, 1, self.texel.ctypes.data))
            d.textures, d.textureCount = C.addressof(self.texture), 1
            self.materials.view(np.uint32)[0, 21] = SCENE_TEXTURE_OFFSET  # the normal slot (include/ptx.h PtxMetallicRoughnessMaterial)
        d.metallicRoughnessMaterials, d.metallicRoughnessMaterialCount = self.materials.ctypes.data, 1
        d.meshes, d.meshCount = self.meshes.ctypes.data, len(self.meshes)
        d.models, d.modelCount = self.models.ctypes.data, len(self.models)
        d.instances, d.instanceCount = self.instances.ctypes.data, len(self.instances)
        self.desc = d

    def pairs(self):
        """(instance, geometry record) per (instance, mesh) pair, in pair order."""
        for i, inst in enumerate(self.instances):
            m = self.models[inst["ModelIndex"]]
            for k in range(m["MeshCount"]):
                rec = self.meshes[m["MeshOffset"] + k]
                yield i, rec, self.geometries[rec["GeometryIndex"]]

    def skin_source(self):
        """Per vertex of the skinned block the animated vertex it is a copy of."""
        src = [np.arange(g["VertexOffset"], g["VertexOffset"] + g["VertexLength"]) for _, _, g in self.pairs() if g["IsAnimated"]]
        return np.concatenate(src) if src else np.zeros(0, np.int64)

    def triangle_class(self):
        """Per global triangle the class label its vertices carry (-1: static geometry or unlabelled)."""
        out = []
        for _, _, g in self.pairs():
            idx = (self.animated_indices if g["IsAnimated"] else self.indices)[g["IndexOffset"]:g["IndexOffset"] + g["IndexLength"]].reshape(-1, 3)
            if g["IsAnimated"]:
                c = self.vertex_class[g["VertexOffset"] + idx.astype(np.int64)]
                assert (c == c[:, 0:1]).all(), "a class sits on its own triangles"
                out.append(c[:, 0])
            else:
                out.append(np.full(len(idx), -1, np.int64))
        return np.concatenate(out)


def posed_vertices(soup, bones, dtype, instance_transforms=None):
    """(block, triangles).  block: the skinned vertex block in the device's order, rows of 14 values in `dtype`: one copy per
    (instance, animated mesh) pair, in pair order (bones = None: the bind pose).  triangles: every triangle of the posed scene in
    world space, float64, (n, 3, 3) in the global order of util.world_triangles."""
    def skinned(dt):
        return bind_vertices(soup.animated_vertices, dt) if bones is None else skin_vertices(soup.animated_vertices, bones, dt)
    block = skinned(dtype)[soup.skin_source()]
    v64 = skinned(np.float64)
    tris = []
    for i, rec, g in soup.pairs():
        x = soup.instances[i]["Transform"] if instance_transforms is None else np.asarray(instance_transforms, np.float32).reshape(-1, 12)[i]
        M = np.vstack([np.float64(x).reshape(3, 4), [0, 0, 0, 1]]) @ np.vstack([np.float64(soup.transforms[rec["TransformIndex"]]).reshape(3, 4), [0, 0, 0, 1]])
        lo, n = int(g["VertexOffset"]), int(g["VertexLength"])
        if g["IsAnimated"]:
            v, idx = v64[lo:lo + n, 0:3], soup.animated_indices
        else:
            v, idx = np.float64(soup.vertices[lo:lo + n, 0:3]), soup.indices
        idx = idx[g["IndexOffset"]:g["IndexOffset"] + g["IndexLength"]].reshape(-1, 3)
        tris.append((v @ M[:3, :3].T + M[:3, 3])[idx])
    return block, (np.concatenate(tris) if tris else np.zeros((0, 3, 3)))
