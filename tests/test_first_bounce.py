"""The first bounce of a launch computes its primary rays (k_trace_closest<.., FIRST>, k_shade<.., FIRST>: csrc/pt_wavefront.hpp,
FirstClosestIO) instead of reading what k_generate wrote.  PTX_FIRST_BOUNCE=0 selects the schedule with k_generate; both must
give the same image and the same statistics bit for bit, and the new one must agree with the oracle on its own."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

W, H = 67, 45  # neither extent a multiple of 8: every edge block has lanes outside the image
SCENES = {"chess_like": 0.05, "texture_test": 1.0, "alpha_test": 1.0}  # kernel modes 0 (opaque), 1 (textured), 2 (any-hit stages)
STAT_FIELDS = ("segments", "shadowRays", "pathSamples", "retries", "tracedRays")

_scenes = {}


def _scene(pkg, name):
    if name not in _scenes:
        _scenes[name] = pkg.Scene(name, SCENES.get(name, 1.0))
    return _scenes[name]


def _stats(r):
    st = r.stats()
    return tuple(int(getattr(st, f)) for f in STAT_FIELDS)


def _run(pkg, monkeypatch, first, scene, lights=None, frames=None, depth=6, lens=0.0, sample_count=1, launches=1, shard=None, before=None):
    """One renderer created under PTX_FIRST_BOUNCE=`first`: `launches` launches (render_frames of `frames` frames, or render
    with `sample_count` samples when frames is None); returns (image as uint32, statistics of every launch)."""
    import torch  # noqa: F401

    monkeypatch.setenv("PTX_FIRST_BOUNCE", "1" if first else "0")
    lights = scene.lights if lights is None else lights
    r = pkg.Renderer()
    r.upload(scene)
    r.resize(W, H)
    if before:
        before(r)
    if shard:
        r.set_tile_shard(*shard)
    stats = []
    for k in range(launches):
        u = scene.uniform(W, H, bounces=depth, sample_count=sample_count, total_samples=k * sample_count, lens_radius=lens, focal_distance=6.0)
        if frames is None:
            r.render(u, lights)
        else:
            r.render_frames(u, lights, k * frames, frames)
        stats.append(_stats(r))
    img = r.readback()
    r.close()
    return img.view(np.uint32), stats


def _same(pkg, monkeypatch, scene, **kw):
    new, new_stats = _run(pkg, monkeypatch, True, scene, **kw)
    old, old_stats = _run(pkg, monkeypatch, False, scene, **kw)
    assert new_stats == old_stats, (new_stats, old_stats)
    assert (new == old).all(), f"{int((new != old).any(axis=-1).sum())} pixels differ"
    return new, new_stats


@pytest.mark.parametrize("depth", [1, 6])
@pytest.mark.parametrize("frames", [1, 3, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_batched_frames_equal_the_schedule_with_k_generate(pkg, monkeypatch, name, frames, depth):
    # frames per wave 1 (1 and 3 frames) and 8; depth 1: the first bounce is also the last
    img, stats = _same(pkg, monkeypatch, _scene(pkg, name), frames=frames, depth=depth)
    assert stats[0][2] == W * H * frames + stats[0][3]  # pathSamples: every pixel of every frame once (+ retries)
    assert img.view(np.float32)[..., :3].max() > 0.0


@pytest.mark.parametrize("name", list(SCENES))
def test_thin_lens_draws_happen_in_both_kernels(pkg, monkeypatch, name):
    _same(pkg, monkeypatch, _scene(pkg, name), frames=3, lens=0.08)


@pytest.mark.parametrize("name", list(SCENES))
def test_multi_sample_launch_first_round_new_kernels_later_rounds_k_restart(pkg, monkeypatch, name):
    _, stats = _same(pkg, monkeypatch, _scene(pkg, name), sample_count=3, launches=2)
    assert stats[0][2] == W * H * 3 + stats[0][3]


@pytest.mark.parametrize("shard", [(1, 3, 32), (0, 1, 32)])
@pytest.mark.parametrize("name", list(SCENES))
def test_dead_slots_of_ragged_tiles_do_not_reach_the_image(pkg, monkeypatch, name, shard):
    # the whole frame is rendered first, so that the slots which are dead under the shard hold a finished radiance from before
    def whole_frame_first(r):
        sc = _scene(pkg, name)
        r.render_frames(sc.uniform(W, H, bounces=4), sc.lights, 0, 2)
        r.reset()

    img, _ = _same(pkg, monkeypatch, _scene(pkg, name), frames=2, shard=shard, before=whole_frame_first)
    mask = pkg.shard_mask(W, H, *shard)
    assert (img[~mask] == 0).all()
    assert (img[mask][..., 3] == np.float32(1.0).view(np.uint32)).all()
    if shard[1] == 1:
        whole, _ = _run(pkg, monkeypatch, True, _scene(pkg, name), frames=2)
        assert (img == whole).all()


@pytest.mark.parametrize("threshold", ["0", "100000000"])
@pytest.mark.parametrize("name", list(SCENES))
def test_k_tail_straight_after_the_first_bounce_finds_a_complete_meta(pkg, monkeypatch, name, threshold):
    # a huge threshold: k_tail takes every path over behind bounce 1 (pixel, frame and RNG state come from the first k_shade)
    monkeypatch.setenv("PTX_TAIL_THRESHOLD", threshold)
    _same(pkg, monkeypatch, _scene(pkg, name), frames=3)
    _same(pkg, monkeypatch, _scene(pkg, name), sample_count=2)


@pytest.mark.parametrize("name", list(SCENES))
def test_sorted_shade_queue_sorts_positions(pkg, monkeypatch, name):
    plain, _ = _run(pkg, monkeypatch, True, _scene(pkg, name), frames=3)
    monkeypatch.setenv("PTX_SHADE_SORT", "1")
    img, _ = _same(pkg, monkeypatch, _scene(pkg, name), frames=3)
    assert (img == plain).all()


@pytest.mark.parametrize("kw", [dict(frames=2, depth=6), dict(frames=2, depth=4, lens=0.08), dict(frames=2, depth=4, sample_count=3)],
                         ids=["plain", "lens", "three_samples"])
@pytest.mark.parametrize("name", list(SCENES))
def test_new_schedule_matches_oracle(pkg, orc, monkeypatch, name, kw):
    monkeypatch.setenv("PTX_FIRST_BOUNCE", "1")
    img, ref = util.render_pair(pkg, orc, name, SCENES[name], W, H, **kw)  # counts are checked launch by launch in there
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_no_dependence_on_the_slot_state_of_an_earlier_launch(pkg, monkeypatch, name):
    import torch  # noqa: F401

    scene = _scene(pkg, name)
    fresh, fresh_stats = _run(pkg, monkeypatch, True, scene, frames=2)
    monkeypatch.setenv("PTX_FIRST_BOUNCE", "1")
    r = pkg.Renderer()
    r.upload(scene)
    r.resize(96, 54)
    r.render_frames(scene.uniform(96, 54, bounces=6), scene.lights, 0, 4)
    r.resize(W, H)
    u = scene.uniform(W, H, bounces=6)
    for attempt in ("host-driven schedule", "hinted schedule"):  # the second launch of a shape is enqueued at once from the hint
        r.reset()
        r.render_frames(u, scene.lights, 0, 2)
        assert [_stats(r)] == fresh_stats, attempt
        assert (r.readback().view(np.uint32) == fresh).all(), attempt
    r.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_borrower_on_its_own_stream_renders_the_owners_image(pkg, monkeypatch, name):
    import torch

    scene = _scene(pkg, name)
    monkeypatch.setenv("PTX_FIRST_BOUNCE", "1")
    u = scene.uniform(W, H, bounces=5)
    owner = pkg.Renderer()
    owner.upload(scene)
    owner.resize(W, H)
    stream = torch.cuda.Stream()
    borrower = pkg.Renderer(stream=stream.cuda_stream)
    borrower.share_scene(owner)
    borrower.resize(W, H)
    owner.render_frames(u, scene.lights, 0, 3)
    borrower.render_frames(u, scene.lights, 0, 3)  # both in flight, each with its own copy of the launch parameters
    a, b = owner.readback(), borrower.readback()
    assert _stats(owner) == _stats(borrower)
    borrower.close()
    owner.close()
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert a[..., :3].max() > 0.0


@pytest.mark.parametrize("threshold", ["0", "100000000", None])
def test_nan_inf_restarts_equal_the_schedule_with_k_generate(pkg, monkeypatch, threshold):
    """The scene and lights of test_nan_inf_samples_restart_like_the_reference: a point light of infinite colour among twelve."""
    if threshold is not None:
        monkeypatch.setenv("PTX_TAIL_THRESHOLD", threshold)
    scene = pkg.Scene("default")
    lights = scene.lights
    lights.LightCount = 12
    for i in range(12):
        for k in range(3):
            lights.Lights[i].Color[k] = float("inf") if i == 0 else 0.0
        lights.Lights[i].Position[0], lights.Lights[i].Position[1], lights.Lights[i].Position[2] = 1.0, -2.0, 0.5
        lights.Lights[i].AttenuationConstant = 1.0
    import torch  # noqa: F401

    NW, NH = 96, 54
    results = {}
    for first in (True, False):
        monkeypatch.setenv("PTX_FIRST_BOUNCE", "1" if first else "0")
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(NW, NH)
        stats = []
        for f, sample_count in enumerate((1, 1, 3)):  # canonical: k_finish_restarts; multi-sample: round by round through k_restart
            r.render(scene.uniform(NW, NH, bounces=4, sample_count=sample_count, total_samples=f), lights)
            stats.append(_stats(r))
        results[first] = (r.readback().view(np.uint32), stats)
        r.close()
    assert results[True][1] == results[False][1]
    assert all(st[3] > 0 for st in results[True][1]), "the scene must provoke restarts"
    assert np.isfinite(results[True][0].view(np.float32)).all()
    assert (results[True][0] == results[False][0]).all()
