"""The GPU side of tests/test_stream_plan_gpu.py, run as a process of its own: GPU_MAX_HW_QUEUES is read when the HIP runtime
initialises, so every queue count needs a fresh process.  Usage: stream_plan_child.py REF.npz -- prints one JSON object
{"failures": [...], "notes": [...]} as its last stdout line (notes: what ptx_create left in ptx_last_error, handle by handle).

Per scene of REF.npz (96 x 64, two launches of one sample, depth 4; oracle image and per-launch counters):
  1. a handle renders ALONE (its two streams fit any queue count >= 4), blocking and pipelined read-back;
  2. three borrowers of its scene join: all four render in flight, each on its own stream -- the first handle's plan may change here;
  3. a PTX_DEVICE_SINGLE_STREAM handle renders the same frames;
  4. (textured scene) borrowers created while the owner's textures are pending render right behind the owner's commit."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402  (first: the HIP library shares torch's runtime)

import __graft_entry__ as graft  # noqa: E402

W, H, DEPTH, LAUNCHES = 96, 64, 4, 2
failures, notes = [], []


def check(cond, what):
    if not cond:
        failures.append(what)


def same(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def counters(r):
    st = r.stats()  # waits for the handle's launch
    return [int(st.segments), int(st.shadowRays), int(st.pathSamples)]


def render_all(scene, handles):
    """LAUNCHES launches on every handle, all handles in flight together; returns the counters [handle][launch]."""
    out = [[] for _ in handles]
    for r in handles:
        r.reset()
    for f in range(LAUNCHES):
        u = scene.uniform(W, H, bounces=DEPTH, sample_count=1, total_samples=f)
        for r in handles:
            r.render(u, scene.lights)
        for k, r in enumerate(handles):
            out[k].append(counters(r))
    return out


def pipelined(r, pinned):
    """ptx_readback_begin / ptx_readback_end into page-locked memory, and into pageable memory (the runtime's copy)."""
    r.readback_begin(pinned.data_ptr(), pinned.numel() * 4)
    r.readback_end()
    a = pinned.numpy().reshape(H, W, 4).copy()
    plain = np.full((H, W, 4), np.nan, np.float32)
    r.readback_begin(plain.ctypes.data, plain.nbytes)
    r.readback_end()
    return a, plain


def check_handle(label, r, got_counters, ref_img, ref_counters, pinned):
    check(got_counters == ref_counters, f"{label}: counters {got_counters} != oracle {ref_counters}")
    a, plain = pipelined(r, pinned)
    img = r.readback()
    check(same(img, ref_img), f"{label}: {int((img.view(np.uint32) != ref_img.view(np.uint32)).any(axis=-1).sum())} pixels differ from the oracle")
    check(same(a, img), f"{label}: readback_begin / readback_end (page-locked) != readback()")
    check(same(plain, img), f"{label}: readback_begin / readback_end (pageable) != readback()")
    return img


def note(pkg, r):
    return r.lib.ptx_last_error(r.handle).decode()


def run_scene(pkg, name, ref_img, ref_counters):
    scene = pkg.Scene(name)
    streams = [torch.cuda.Stream()]
    a = pkg.Renderer(stream=streams[0].cuda_stream)
    a.upload(scene)
    a.resize(W, H)
    pinned = torch.empty(W * H * 4, dtype=torch.float32, pin_memory=True)
    alone = check_handle(f"{name}/alone", a, render_all(scene, [a])[0], ref_img, ref_counters, pinned)
    # (asked after the first launch: the statistics of a handle that never rendered read events that were never recorded)
    check(a.stats().hardwareQueues == int(os.environ["GPU_MAX_HW_QUEUES"]), f"hardwareQueues {a.stats().hardwareQueues}")
    others = []
    for _ in range(3):
        streams.append(torch.cuda.Stream())
        b = pkg.Renderer(stream=streams[-1].cuda_stream)
        notes.append(note(pkg, b))
        b.share_scene(a)
        b.resize(W, H)
        others.append(b)
    got = render_all(scene, [a] + others)
    for k, r in enumerate([a] + others):
        img = check_handle(f"{name}/four in flight/handle {k}", r, got[k], ref_img, ref_counters, pinned)
        check(same(img, alone), f"{name}: handle {k} among four differs from the handle alone")
    # once more: the hinted schedule (the second launch of a shape is enqueued at once), all read-backs pipelined and in flight together
    render_all(scene, [a] + others)
    frames = [torch.empty(W * H * 4, dtype=torch.float32, pin_memory=True) for _ in range(4)]
    for r, f in zip([a] + others, frames):
        r.readback_begin(f.data_ptr(), W * H * 16)
    for k, (r, f) in enumerate(zip([a] + others, frames)):
        r.readback_end()
        check(same(f.numpy().reshape(H, W, 4), ref_img), f"{name}: pipelined read-back of handle {k} (hinted launch) differs from the oracle")
    single = pkg.Renderer(single_stream=True)
    single.share_scene(a)
    single.resize(W, H)
    check_handle(f"{name}/single-stream handle", single, render_all(scene, [single])[0], ref_img, ref_counters, pinned)
    single.close()
    for b in others:  # the first handle is alone again: its plan may change back
        b.close()
    check_handle(f"{name}/alone again", a, render_all(scene, [a])[0], ref_img, ref_counters, pinned)
    a.close()
    scene.close()


def run_commit(pkg, ref_img, ref_counters):
    """Borrowers render right behind the owner's texture commit, with nothing waited for in between."""
    import test_texture_streaming as tts

    ts = tts._TexturedScene(pkg, "texture_test")
    owner = pkg.Renderer()
    owner.upload_streamed(ts.pending(), ts.stand_in)
    borrowers = []
    streams = [torch.cuda.Stream() for _ in range(3)]
    for s in streams:
        b = pkg.Renderer(stream=s.cuda_stream)
        b.share_scene(owner)
        b.resize(W, H)
        borrowers.append(b)
    u = ts.scene.uniform(W, H, bounces=DEPTH, sample_count=1, total_samples=0)
    for b in borrowers:  # a frame with the stand-ins first: the streams exist and are busy
        b.render(u, ts.scene.lights)
    tts._upload_all(pkg, owner, ts.full, range(ts.n))
    check(owner.commit_textures() == ts.n, "commit count")
    got = render_all(ts.scene, borrowers)
    for k, b in enumerate(borrowers):
        check(got[k] == ref_counters, f"commit: borrower {k} counters {got[k]} != oracle {ref_counters}")
        check(same(b.readback(), ref_img), f"commit: borrower {k} did not render the committed textures")
        b.close()
    owner.close()


def main():
    ref = np.load(sys.argv[1])
    torch.cuda.set_device(0)
    pkg = graft.load_package()
    for name in ("default", "texture_test"):
        run_scene(pkg, name, ref[name + "_img"], ref[name + "_counters"].tolist())
    run_commit(pkg, ref["texture_test_img"], ref["texture_test_counters"].tolist())
    print(json.dumps({"failures": failures, "notes": notes}))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
