"""Where a path's state lives between two kernels (csrc/pt_wavefront.hpp, struct Wavefront).  The RNG state and bounce | smpl << 16
have no record of their own: they ride in thr.w and rayD.w, in shC.w and rayO.w for a path that ended with its shadow query
pending; pixel and frame are recomputed from the slot; the shadow ray takes its origin from rayO and carries the finished flag
as the sign bit of its length.  None of that may show: every image here is the oracle's bit for bit, with the oracle's counts,
on every route a slot can take from one kernel to the next."""
import os
import subprocess
import sys

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

W, H = 67, 45  # neither extent a multiple of 8: every edge block has lanes outside the image
SCENES = {"chess_like": 0.05, "texture_test": 1.0, "alpha_test": 1.0}  # kernel modes 0 (opaque), 1 (textured), 2 (any-hit stages)
COUNTS = ("segments", "shadowRays", "pathSamples", "retries")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_scenes, _oracles, _refs = {}, {}, {}


def _scene(pkg, name):
    if name not in _scenes:
        _scenes[name] = pkg.Scene(name, SCENES[name])
    return _scenes[name]


def _uniform(scene, w, h, depth, sample_count, frame, lens):
    return scene.uniform(w, h, bounces=depth, sample_count=sample_count, total_samples=frame * sample_count, lens_radius=lens, focal_distance=6.0)


def _reference(pkg, orc, name, frames=1, depth=8, sample_count=1, lens=0.0, w=W, h=H):
    """The oracle's accumulation image after `frames` launches of `sample_count` samples, and its counts summed over them.
    Computed once per case and shared; nobody writes into it."""
    key = (name, frames, depth, sample_count, lens, w, h)
    if key not in _refs:
        scene = _scene(pkg, name)
        if name not in _oracles:
            _oracles[name] = orc.OracleScene(scene.desc, build_bvh=True)
        ref = np.zeros((h, w, 4), np.float32)
        counts = np.zeros(len(COUNTS), np.int64)
        for f in range(frames):
            _, st = _oracles[name].render(_uniform(scene, w, h, depth, sample_count, f, lens), scene.lights, w, h, accum=ref)
            counts += [int(getattr(st, c)) for c in COUNTS]
        ref.setflags(write=False)
        _refs[key] = (ref, tuple(int(c) for c in counts))
    return _refs[key]


def _counts(st):
    return tuple(int(getattr(st, c)) for c in COUNTS)


def _render(pkg, name, frames=1, depth=8, sample_count=1, lens=0.0, w=W, h=H, backend=None, shard=None):
    """One launch on a fresh renderer: render_frames of `frames` canonical frames, or render with `sample_count` samples.
    Returns (image, counts, statistics)."""
    import torch  # noqa: F401

    scene = _scene(pkg, name)
    r = pkg.Renderer(backend=pkg.BACKEND_WAVEFRONT if backend is None else backend)
    r.upload(scene)
    r.resize(w, h)
    if shard:
        r.set_tile_shard(*shard)
    u = _uniform(scene, w, h, depth, sample_count, 0, lens)
    if sample_count == 1:
        r.render_frames(u, scene.lights, 0, frames)
    else:
        assert frames == 1
        r.render(u, scene.lights)
    img, st = r.readback(), r.stats()
    r.close()
    return img, _counts(st), st


def _differing(img, ref):
    return int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())


def _check(pkg, orc, name, megakernel=True, **kw):
    ref, want = _reference(pkg, orc, name, **kw)
    img, got, st = _render(pkg, name, **kw)
    assert got == want, (got, want)
    assert _differing(img, ref) == 0, f"wavefront: {_differing(img, ref)} pixels differ from the oracle"
    assert ref[..., :3].max() > 0.0
    if megakernel:
        mega, got, _ = _render(pkg, name, backend=pkg.BACKEND_MEGAKERNEL, **kw)
        assert got == want and _differing(mega, img) == 0
    return st


@pytest.mark.parametrize("frames", [8, 3])  # frames per wave 8 and 1: the two branches of the slot -> (frame, pixel) mapping
@pytest.mark.parametrize("name", list(SCENES))
def test_canonical_launch(pkg, orc, name, frames):
    _check(pkg, orc, name, frames=frames, depth=8)


@pytest.mark.parametrize("lens", [0.0, 0.08], ids=["pinhole", "lens"])  # the lens adds two draws per sample
@pytest.mark.parametrize("depth", [1, 8])  # depth 1: every path ends in k_shade or in k_apply_shadow
@pytest.mark.parametrize("name", list(SCENES))
def test_multi_sample_launch_carries_the_rng_through_two_restarts(pkg, orc, name, depth, lens):
    st = _check(pkg, orc, name, depth=depth, sample_count=3, lens=lens)
    assert st.pathSamples == 3 * W * H + st.retries


def test_k_tail_takes_over_what_k_shade_wrote(pkg, orc, monkeypatch):
    """k_tail reads thr.w / rayD.w of slots the shade kernel of the bounce before it left.  Two situations, told apart by the
    statistics: traceLaunches counts two per bounce the wavefront kernels ran, segments - tracedRays is what k_tail traced."""
    # 24,120 slots: the queue the first bounce leaves is below the default threshold (75,000) at once
    monkeypatch.delenv("PTX_TAIL_THRESHOLD", raising=False)  # the default, whatever the environment carries
    st = _check(pkg, orc, "chess_like", frames=8, depth=8, megakernel=False)
    assert st.traceLaunches == 2 and st.segments > st.tracedRays
    # 115,200 slots and a threshold of 3,000: the tail takes over behind the third bounce or later
    monkeypatch.setenv("PTX_TAIL_THRESHOLD", "3000")
    st = _check(pkg, orc, "chess_like", frames=8, depth=8, w=160, h=90, megakernel=False)
    assert st.traceLaunches >= 6 and st.segments > st.tracedRays
    # and with no tail at all every bounce is the wavefront's
    monkeypatch.setenv("PTX_TAIL_THRESHOLD", "0")
    st = _check(pkg, orc, "chess_like", frames=8, depth=8, megakernel=False)
    assert st.traceLaunches > 2 and st.segments == st.tracedRays


@pytest.mark.parametrize("name", list(SCENES))
def test_ragged_tile_shard_recomputes_the_pixel_from_the_slot(pkg, orc, name):
    # rank 1 of 3 at tile 32: slots outside the image (dead for the whole launch), and k_restart starts the second sample of
    # every live slot at a pixel it has to work out from the slot index
    shard = (1, 3, 32)
    ref, _ = _reference(pkg, orc, name, depth=8, sample_count=2)
    img, got, _ = _render(pkg, name, depth=8, sample_count=2, shard=shard)
    mask = pkg.shard_mask(W, H, *shard)
    assert 0 < mask.sum() < W * H
    assert got[2] == 2 * int(mask.sum()) + got[3]
    assert (img.view(np.uint32)[mask] == ref.view(np.uint32)[mask]).all()
    assert (img.view(np.uint32)[~mask] == 0).all()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
import __graft_entry__ as graft
pkg = graft.load_package()
W, H = 67, 45
out = {}
for name, detail in (("chess_like", 0.05), ("texture_test", 1.0), ("alpha_test", 1.0)):
    scene = pkg.Scene(name, detail)
    for tag, depth, shard in (("d1", 1, None), ("d8", 8, None), ("shard", 8, (1, 3, 32))):
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(W, H)
        if shard:
            r.set_tile_shard(*shard)
        r.render(scene.uniform(W, H, bounces=depth, sample_count=3, total_samples=0, lens_radius=0.0, focal_distance=6.0), scene.lights)
        out[name + "_" + tag] = r.readback()
        st = r.stats()
        out[name + "_" + tag + "_counts"] = np.array([st.segments, st.shadowRays, st.pathSamples, st.retries], np.int64)
        r.close()
np.savez(sys.argv[2], **out)
"""


def test_schedule_with_k_generate_in_a_child_process(pkg, orc, tmp_path):
    """PTX_FIRST_BOUNCE=0: k_generate writes thr.w / rayD.w of every slot and flags the slots outside the image in rayD.w, the
    general kernels read them at bounce 0.  The multi-sample launches above, and the ragged shard, in a process of their own."""
    env = dict(os.environ, PTX_FIRST_BOUNCE="0")
    out = tmp_path / "k_generate.npz"
    done = subprocess.run([sys.executable, "-c", _CHILD, REPO, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(out)
    mask = pkg.shard_mask(W, H, 1, 3, 32)
    for name in SCENES:
        for tag, depth in (("d1", 1), ("d8", 8)):
            ref, want = _reference(pkg, orc, name, depth=depth, sample_count=3)
            assert tuple(int(c) for c in got[f"{name}_{tag}_counts"]) == want, (name, tag)
            assert _differing(got[f"{name}_{tag}"], ref) == 0, (name, tag)
        ref, _ = _reference(pkg, orc, name, depth=8, sample_count=3)
        img = got[f"{name}_shard"]
        assert (img.view(np.uint32)[mask] == ref.view(np.uint32)[mask]).all() and (img.view(np.uint32)[~mask] == 0).all(), name


# ---------------------------------------------------------------------------------------
# the shadow record: visible / occluded x the path ends here / goes on
# ---------------------------------------------------------------------------------------
def _two_quads(pkg):
    """A floor that fills the view and a small quad above it; the camera looks down at both: every primary ray hits."""
    floor = util.quad_mesh([[-12, 0, 12], [12, 0, 12], [12, 0, -12], [-12, 0, -12]], [0, 1, 0])
    occluder = util.quad_mesh([[-1, 1, 1], [1, 1, 1], [1, 1, -1], [-1, 1, -1]], [0, 1, 0])
    soup = util.TriangleSoup(pkg, [[floor], [occluder]], material=util.mr_material(color=(0.8, 0.6, 0.4), roughness=0.6))
    cam = pkg.Scene("default", 0.05)
    cam.set_camera_pose((0.0, 6.0, 5.0), (0.0, -0.8, -0.5))
    return soup, cam


def _shadow_lights(pkg, kind):
    """Both lights stand above the floor, so every hit asks its query (the contribution is never zero).  "directional": that
    light alone, LightDistance = 100000; "point": one point light beside it, LightDistance = the distance to it; "nan": the point
    light beside a directional light of direction 0 -- selecting that one gives a NaN sample, which is restarted.
    (Why "point" keeps a lit directional light: light selection always draws among LightCount + 1 lights.  A directional light
    without colour would be selected by half the hits and give them a zero contribution, for which no query is made -- a black
    pixel at depth 1 would then no longer mean "occluded", which is what the test reads the finished-and-occluded count from.)"""
    lights = pkg.LightsUbo()
    lights.Directional.Color[:] = (3.0, 2.5, 2.0)
    lights.Directional.Direction[:] = (0.0, 0.0, 0.0) if kind == "nan" else (0.1, -1.0, 0.05)
    if kind != "directional":
        lights.LightCount = 1
        lights.Lights[0].Color[:] = (40.0, 40.0, 50.0)
        lights.Lights[0].Position[:] = (0.2, 4.0, 0.1)
        lights.Lights[0].AttenuationConstant, lights.Lights[0].AttenuationLinear, lights.Lights[0].AttenuationQuadratic = 1.0, 0.1, 0.02
    return lights


def _soup_pair(pkg, orc, soup, cam, lights, depth, sample_count=1):
    import torch  # noqa: F401

    u = cam.uniform(W, H, bounces=depth, sample_count=sample_count)
    osc = orc.OracleScene(soup.desc, build_bvh=True)
    ref, ost = osc.render(u, lights, W, H)
    osc.close()
    r = pkg.Renderer()
    r.upload(soup.desc)
    r.resize(W, H)
    r.render(u, lights)
    img, st = r.readback(), r.stats()
    r.close()
    assert _counts(st) == _counts(ost), (_counts(st), _counts(ost))
    assert _differing(img, ref) == 0, f"{_differing(img, ref)} pixels differ from the oracle"
    return img, st


@pytest.mark.parametrize("kind", ["point", "directional"])
def test_shadow_record_all_four_outcomes(pkg, orc, kind):
    soup, cam = _two_quads(pkg)
    lights = _shadow_lights(pkg, kind)
    # depth 1: every path ends at its first hit, so every shadow query belongs to a finished path.  Nothing is emissive and
    # no ray reaches the sky: a pixel is black exactly if its query was occluded (or none was made), lit if the light was visible.
    one, st1 = _soup_pair(pkg, orc, soup, cam, lights, 1)
    assert st1.pathSamples == W * H and st1.shadowRays == W * H and st1.segments == W * H and st1.retries == 0
    lit1 = one[..., :3].max(axis=-1) > 0.0
    finished_visible, finished_occluded = int(lit1.sum()), int((~lit1).sum())
    # depth 8, same frame: the RNG stream of a path is the same up to the end of its first bounce, so its first query has the
    # same answer.  A pixel whose value changed belongs to a path that went on behind that query and found more light.
    many, st8 = _soup_pair(pkg, orc, soup, cam, lights, 8)
    assert st8.pathSamples == W * H and st8.shadowRays > st1.shadowRays and st8.segments > W * H
    changed = (many.view(np.uint32) != one.view(np.uint32)).any(axis=-1)
    continuing_visible, continuing_occluded = int((changed & lit1).sum()), int((changed & ~lit1).sum())
    print(f"{kind}: finished visible / occluded {finished_visible} / {finished_occluded}, continuing visible / occluded "
          f"{continuing_visible} / {continuing_occluded}; closest hits {st1.shadowRays} -> {st8.shadowRays}, segments {st8.segments}")
    assert min(finished_visible, finished_occluded, continuing_visible, continuing_occluded) >= 10
    assert (many[..., :3] >= one[..., :3]).all()
    # two samples per launch: the paths that end in k_apply_shadow hand RNG state and sample index to k_restart
    _, st = _soup_pair(pkg, orc, soup, cam, lights, 8, sample_count=2)
    assert st.pathSamples == 2 * W * H


@pytest.mark.parametrize("sample_count", [1, 2])  # k_finish_restarts; round by round through k_restart
def test_nan_restarts_find_the_rng_state_in_the_shadow_record(pkg, orc, sample_count):
    """Half of the samples select a light whose direction is NaN: they end (depth 1: all of them in k_apply_shadow or k_shade)
    and start again with the RNG carried on, until the other light is drawn."""
    soup, cam = _two_quads(pkg)
    for depth in (1, 8):
        _, st = _soup_pair(pkg, orc, soup, cam, _shadow_lights(pkg, "nan"), depth, sample_count=sample_count)
        assert st.retries > W * H // 4  # (a NaN restarts ALL samples of its launch: the counts are the oracle's, checked in there)


def test_checkpoint_and_resume_equal_the_uninterrupted_render(pkg, tmp_path):
    import torch  # noqa: F401

    scene = _scene(pkg, "chess_like")
    u = scene.uniform(W, H, bounces=8)

    def renderer():
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(W, H)
        return r

    a = renderer()
    a.render_frames(u, scene.lights, 0, 3)
    pkg.save_checkpoint(tmp_path / "half.ptxacc", a.readback(), 3)
    a.render_frames(u, scene.lights, 3, 3)
    full = a.readback()
    a.close()
    b = renderer()
    acc, n = pkg.load_checkpoint(tmp_path / "half.ptxacc")
    b.write_accumulation(acc)
    b.render_frames(u, scene.lights, n, 3)
    resumed = b.readback()
    b.close()
    assert n == 3 and _differing(resumed, full) == 0
