"""ptx_scene_upload refuses before it touches the handle: a description that is refused with PTX_ERROR_INVALID_ARGUMENT, for
whatever reason, leaves an owner with its scene and a borrower borrowing (csrc/pt_scene_host.hpp: validateSceneDesc,
flattenScene and planTextures finish before the old scene goes).  Beside that, the accepted upload whose textures are scaled
through the scratch chains of the upload-format pools, which live for that one call."""
import ctypes as C

import numpy as np
import pytest

W, H = 64, 48


class _TextureDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("levels", C.c_uint32), ("data", C.c_void_p)]


class _Rig:
    """One owner and one borrower of `name`'s scene, and the bits of the frame both render."""

    def __init__(self, pkg, name):
        self.scene = pkg.Scene(name)
        self.u = self.scene.uniform(W, H, bounces=3)
        self.owner, self.borrower = pkg.Renderer(), pkg.Renderer()
        self.owner.upload(self.scene)
        self.borrower.share_scene(self.owner)
        for r in (self.owner, self.borrower):
            r.resize(W, H)
        self.frame = self.render(self.owner)
        assert (self.render(self.borrower) == self.frame).all()
        self.triangles = self.owner.stats().triangles

    def render(self, r):
        r.reset()
        r.render_frames(self.u, self.scene.lights, 0, 1)
        return r.readback().view(np.uint32)

    def close(self):
        self.borrower.close()
        self.owner.close()


@pytest.fixture(scope="module")
def rigs(pkg):
    import torch  # noqa: F401

    r = {"texture_test": _Rig(pkg, "texture_test"), "reuse_mesh_cubes": _Rig(pkg, "reuse_mesh_cubes")}
    yield r
    for rig in r.values():
        rig.close()


def _copy(desc):
    bad = type(desc)()
    C.memmove(C.byref(bad), C.byref(desc), C.sizeof(bad))
    return bad


def _table(address, count):
    src = (_TextureDesc * count).from_address(address)
    arr = (_TextureDesc * count)()
    C.memmove(arr, src, C.sizeof(arr))
    return arr


def _sky_kind_3(desc):
    bad = _copy(desc)
    sky = (_TextureDesc * 1)(_TextureDesc(1, 1, 1, 1, None))  # the kind counts only for a description that has sky images
    bad.skybox, bad.skyboxKind = C.addressof(sky), 3
    return bad, sky


def _cube_face_3_wider(desc):
    assert desc.skyboxKind == 2
    bad = _copy(desc)
    sky = _table(desc.skybox, 6)
    sky[3].width += 1
    bad.skybox = C.addressof(sky)
    return bad, sky


def _format_7(desc):
    bad = _copy(desc)
    tex = _table(desc.textures, desc.textureCount)
    tex[0].format = 7
    bad.textures = C.addressof(tex)
    return bad, tex


def _five_levels_of_2x2(desc):
    bad = _copy(desc)
    tex = _table(desc.textures, desc.textureCount)
    tex[0].width, tex[0].height, tex[0].levels = 2, 2, 5
    bad.textures = C.addressof(tex)
    return bad, tex


def _two_to_the_29_triangles(desc):
    """One geometry of 65,536 triangles, instanced 8,192 times: 2^29 triangles against a limit of 2^29 - 1."""
    bad = _copy(desc)
    vertices = np.zeros((3, 14), np.float32)  # PtxVertex: 56 B
    vertices[1, 0] = vertices[2, 1] = 1.0
    indices = np.tile(np.arange(3, dtype=np.uint32), 65536)
    geometry = np.array([0, 3, 0, indices.size, 1], np.uint32)  # offsets and lengths; IsOpaque = 1, IsAnimated = 0
    material = np.frombuffer((C.c_uint32 * 3).from_address(desc.meshes), np.uint32)[1]
    mesh = np.array([0, material, 0], np.uint32)
    model = np.array([0, 1], np.uint32)
    instances = np.zeros((8192, 13), np.float32)  # PtxModelInstance: ModelIndex 0 + the identity as 3 x 4 floats
    instances[:, 1] = instances[:, 6] = instances[:, 11] = 1.0
    bad.vertices, bad.vertexCount = vertices.ctypes.data, 3
    bad.indices, bad.indexCount = indices.ctypes.data, indices.size
    bad.geometries, bad.geometryCount = geometry.ctypes.data, 1
    bad.meshes, bad.meshCount = mesh.ctypes.data, 1
    bad.models, bad.modelCount = model.ctypes.data, 1
    bad.instances, bad.instanceCount = instances.ctypes.data, 8192
    return bad, (vertices, indices, geometry, mesh, model, instances)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,defect,message", [
    ("texture_test", _sky_kind_3, "unknown skybox kind 3"),
    ("reuse_mesh_cubes", _cube_face_3_wider, "cube skybox"),
    ("texture_test", _format_7, "texture 0: unknown format 7"),
    ("texture_test", _five_levels_of_2x2, "texture 0: 5 levels for a 2 x 2 image"),
    ("texture_test", _two_to_the_29_triangles, "scene has 536870912 triangles"),
], ids=["sky_kind_3", "cube_face_3_wider", "format_7", "five_levels_of_2x2", "two_to_the_29_triangles"])
def test_refused_upload_leaves_owner_and_borrower_as_they_were(pkg, rigs, scene, defect, message):
    rig = rigs[scene]
    bad, keep = defect(rig.scene.desc)
    for r in (rig.owner, rig.borrower):
        with pytest.raises(pkg.PtxError, match=message):
            r._check(r.lib.ptx_scene_upload(r.handle, C.byref(bad)))
        # no new upload, no build: the handle renders what it rendered before, the borrower still from its owner
        assert (rig.render(r) == rig.frame).all()
        assert r.stats().triangles == rig.triangles
    del keep


@pytest.mark.gpu
def test_upload_scaled_through_scratch_chains_matches_oracle(pkg, orc, rigs):
    """A budget of 7,200 B for seven textures (the smallest test_upload_rules_match_oracle_bitexact uploads with) leaves 1,028 B
    each: 8 x 8 is the largest RGBA8 extent (chain of 8: 340 B, of 16: 1,364 B), 4 x 4 the largest RGBA32F one, so the scene's
    level-0-only images go through the scratch chains."""
    rig = rigs["texture_test"]
    d = type(rig.scene.desc).from_buffer_copy(rig.scene.desc)
    d.textureMemoryBudget = 6 * 6000 // 5
    r = pkg.Renderer()
    r.upload(d)
    r.resize(W, H)
    img = rig.render(r)
    r.close()
    ref, _ = orc.OracleScene(d).render(rig.u, rig.scene.lights, W, H)
    assert (img == ref.view(np.uint32)).all()
    assert not (img == rig.frame).all()  # the squeezed textures show
