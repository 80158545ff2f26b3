"""The stream plan (csrc/pt_stream_plan.hpp) never changes an image: with the hardware queues scarce (4: four handles' streams do not
fit, auxiliary kernels and read-back ride the main stream) or plentiful (16: the two-stream schedule), and with PTX_STREAM_PLAN=0,
images and segment / shadow-ray / sample counters are the oracle's bit for bit, the pipelined read-back equals the blocking one, a
handle that rendered alone and is joined by three others renders the same frames before and after, a single-stream handle and a
borrower behind its owner's texture commit do too.  GPU_MAX_HW_QUEUES is read when the HIP runtime starts: every case is a child
process (tests/stream_plan_child.py), one at a time, with its own time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, DEPTH, LAUNCHES = 96, 64, 4, 2  # the child's shape
SCENES = ("default", "texture_test")  # k_tail<0> and k_tail<1>; both finish inside the tail at this size


@pytest.fixture(scope="module")
def oracle_file(pkg, orc, tmp_path_factory):
    """The oracle's image and per-launch counters of every scene, computed once for all cases."""
    out = {}
    for name in SCENES:
        scene = pkg.Scene(name)
        osc = orc.OracleScene(scene.desc, build_bvh=True)
        ref = np.zeros((H, W, 4), np.float32)
        counters = []
        for f in range(LAUNCHES):
            _, st = osc.render(scene.uniform(W, H, bounces=DEPTH, sample_count=1, total_samples=f), scene.lights, W, H, accum=ref)
            counters.append([int(st.segments), int(st.shadowRays), int(st.pathSamples)])
        osc.close()
        scene.close()
        assert ref[..., :3].max() > 0.0
        out[name + "_img"], out[name + "_counters"] = ref, np.array(counters, np.int64)
    path = str(tmp_path_factory.mktemp("stream_plan") / "oracle.npz")
    np.savez(path, **out)
    return path


def _child(oracle_file, queues, plan):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(queues))
    env.pop("PTX_VERBOSE", None)
    env.pop("PTX_STREAM_PLAN", None)
    if plan is not None:
        env["PTX_STREAM_PLAN"] = plan
    p = subprocess.run([sys.executable, os.path.join(HERE, "stream_plan_child.py"), oracle_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, env=env, timeout=120)
    lines = p.stdout.strip().splitlines()
    assert p.returncode in (0, 1) and lines and lines[-1].startswith("{"), f"the child ended with {p.returncode}:\n{p.stderr[-3000:]}"
    res = json.loads(lines[-1])
    assert not res["failures"], res["failures"]
    assert p.returncode == 0
    return res["notes"]


def test_scarce_queues_one_stream_plan_same_frames(oracle_file):
    notes = _child(oracle_file, 4, None)
    # the third handle is the first whose streams no longer fit four queues: its note names the plan it got (from there on the first
    # handle, which rendered alone on two streams, is on the one-stream plan too, and back on two when the others have gone:
    # csrc/pt_stream_plan.hpp is a function of the live handles, tests/test_stream_plan.py)
    assert sum("share 4 hardware queues; stream plan: one stream" in n for n in notes) == 1, notes


def test_plentiful_queues_keep_the_two_stream_schedule(oracle_file):
    notes = _child(oracle_file, 16, None)
    assert not any(notes), notes


def test_switch_off_keeps_two_streams_on_scarce_queues(oracle_file):
    notes = _child(oracle_file, 4, "0")
    assert sum("share 4 hardware queues; stream plan: two streams" in n for n in notes) == 1, notes
