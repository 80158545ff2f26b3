"""A handle's whole life, over and over: every resource a handle makes lazily -- the auxiliary stream and the bounce events of the
first render, the copy stream and snapshot events of the pipelined read-back, the images of the interactive chain and of the screen
path, the staging of ptx_trace_rays and ptx_test_eval, a borrowed scene, a single-stream handle whose auxiliary stream IS its main
one -- is a member that releases itself (csrc/pt_owned.hpp, DevBuf), and ptx_destroy names none of them.  So create / destroy
cycles lose no device memory, compute the same image every time, and an owner that goes first leaves its borrower without a scene,
not with dangling pointers.  And the numbers ptx_get_stats reports about the tree are those of the tree in use, also where
ptx_build_accel built several candidates and swapped whole trees about."""
import numpy as np
import pytest
import util

W, H = 40, 24  # two 32 x 8 tiles across, the second ragged, three down


def _cycle(pkg, scene):
    """One owner, one borrower, one single-stream handle, everything used once; the owner is closed first.
    Returns the images: the owner's through the pinned read-back, the borrower's, the single-stream handle's."""
    import torch

    u, lights = scene.uniform(W, H, bounces=3), scene.lights
    view, proj = scene.camera_matrices(W, H)
    owner = pkg.Renderer()
    owner.upload(scene)
    owner.resize(W, H)
    owner.render_frames(u, lights, 0, 2)  # the auxiliary stream, the bounce events
    host = torch.zeros((H, W, 4), dtype=torch.float32).pin_memory()
    owner.readback_begin(host.data_ptr(), host.numel() * 4)  # the copy stream or the auxiliary one, the snapshot events
    owner.readback_end()
    owner.render_guides(u)
    owner.temporal_accumulate(2, view, proj)
    owner.denoise_temporal()
    owner.postprocess_denoised()
    owner.present(W, H)
    hits, ids = owner.trace_rays(util.random_rays(np.random.default_rng(0), 64, -2.0, 2.0))
    fn = pkg.FN["sqrt"]
    owner.test_eval(fn, np.full((4, owner.lib.ptx_test_input_stride(fn)), 2.0, np.float32))
    borrower = pkg.Renderer()
    borrower.share_scene(owner)
    borrower.resize(W, H)
    borrower.render_frames(u, lights, 0, 1)
    single = pkg.Renderer(single_stream=True)
    single.upload(scene)
    single.resize(W, H)
    single.render_frames(u, lights, 0, 1)
    images = (host.numpy().copy(), borrower.readback(), single.readback(), hits, ids)
    owner.close()
    with pytest.raises(pkg.PtxError):  # the owner went first: no scene, and no dangling pointers
        borrower.render_frames(u, lights, 1, 1)
    borrower.close()
    single.close()
    return images


@pytest.mark.gpu
def test_create_destroy_cycles_lose_no_memory_and_render_the_same_image(pkg):
    import torch

    scene = pkg.Scene("default")
    first = _cycle(pkg, scene)  # first use also pays one-off runtime allocations
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        last = _cycle(pkg, scene)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"{(free0 - free1) / 2**20:.1f} MiB lost over 6 create / destroy cycles")
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) / 2**20:.1f} MiB lost over 6 create / destroy cycles"
    assert np.isfinite(first[0]).all() and first[0].any()  # (a frame was rendered at all)
    for a, b in zip(first, last):
        assert a.dtype == b.dtype and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.gpu
def test_stats_describe_the_tree_in_use_after_a_build_with_candidates(pkg):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    scene = pkg.Scene("chess_like", 0.05)
    assert scene.triangle_count >= 4096  # below that ptx_build_accel builds ONE tree and swaps nothing
    seen = []
    for _ in range(2):
        r = pkg.Renderer()
        r.upload(scene)  # ptx_scene_upload + ptx_build_accel
        st = r.stats()
        print(f"triangles {st.triangles}, treeTriangles {st.treeTriangles}, treeReferences {st.treeReferences}, bvhNodes {st.bvhNodes}")
        assert st.bvhNodes > 0
        assert st.treeReferences >= st.treeTriangles > 0
        assert st.treeTriangles <= st.triangles
        seen.append(st.treeTriangles)
        r.close()
    assert seen[0] == seen[1]
