"""The bookkeeping of the interactive chain (csrc/pt_chain_state.hpp: ChainStatus; csrc/pt_chain_host.hpp): what is ready, which
ping-pong copy is current, when the moments are live and which pose a history leads back to.

`Model` below is that bookkeeping once more, written from the wording of include/ptx.h and docs/NEXT_ROWS.md sections 13, 14, 16 and 17
(each rule cites its sentence), not from the header.

Without a GPU: a stand-alone program that includes pt_chain_state.hpp alone, plain and under the address / undefined-behaviour
sanitizers, reads event sequences and prints the whole status after every event; every sequence of up to four events over an
alphabet of fourteen is compared with the model line by line.

On the GPU, at 40 x 24 (two 32 x 8 tiles across, the second ragged, three down): a dozen call sequences on real handles that pass
every site which resets chain state, with the code of every call, the four device pointers and the two read-backs' refusals held
against the model; and the shared refusal ladder, state by state and entry point by entry point, against the messages written out."""
import itertools
import os
import re
import subprocess

import pytest

W, H = 40, 24
OK, INVALID, NOT_READY = 0, 1, 5  # PTX_OK, PTX_ERROR_INVALID_ARGUMENT, PTX_ERROR_NOT_READY


# =====================================================================================================
# the model
# =====================================================================================================

class PoseModel:
    """POSE BOOKKEEPING of include/ptx.h, kept with the scene: the serial, tracking, and whether the snapshot holds serial - 1"""

    def __init__(self):
        self.serial, self.tracking, self.snapshot = 0, False, False

    def update(self):
        """'The POSE SERIAL S counts the accepted ptx_update_animation calls, tracking or not ... While tracking is on,
        ptx_update_animation first SNAPSHOTS the pose it is about to replace'"""
        self.serial += 1
        self.snapshot = self.tracking

    def track(self, enable):
        """'turning tracking off releases them'"""
        if not enable:
            self.snapshot = False
        self.tracking = enable

    def upload(self):
        """'ptx_scene_upload and its streamed form reset everything: tracking off, no snapshot, and a serial no earlier history leads
        back to' (section 17: 'moves the serial by two')"""
        self.serial += 2
        self.tracking = self.snapshot = False


class Model:
    """One handle's chain.  None stands for 'no pose' and for 'no copy'."""

    def __init__(self, pose=None):
        self.pose = pose or PoseModel()
        self.image = self.usable = False  # ptx_resize; a scene and a tree
        self.bound, self.world = False, 1  # ptx_bind_shard_accumulation; ptx_set_tile_shard's worldSize
        self.guides = self.motion = False
        self.denoised_in = self.history_in = None
        self.temporal = self.moments = self.variance = False
        self.guides_pose = self.temporal_pose = self.motion_from = None

    # ---- what the text calls by name ----
    def history_pose(self):
        """'the pose serial of this renderer's current temporal history'; without a history there is none"""
        return self.temporal_pose if self.history_in is not None else None

    def motion_fresh(self):
        """section 17: 'The motion images belong to the guides they were rendered with and to the history as it stood: after a plain
        ptx_render_guides, or once an accumulate call has moved the history to another pose, the call answers PTX_ERROR_NOT_READY'"""
        return self.motion and self.motion_from == self.history_pose()

    def moments_current(self):
        """'unless the last accepted accumulate call since ptx_resize was ptx_temporal_accumulate_moments'"""
        return self.temporal and self.moments

    def prev_pose(self):
        """ptx_render_guides_motion: 'h == S: the previous pose is the current one; h == S - 1 and the snapshot is valid: the previous
        pose is the snapshot; anything else (no history, several updates since, tracking enabled after the update): UNKNOWN'"""
        h, s = self.history_pose(), self.pose.serial
        if h == s:
            return "current"
        return "snapshot" if h is not None and h + 1 == s and self.pose.snapshot else "unknown"

    # ---- the events ----
    def resize(self):
        """'no ptx_render_guides / ptx_denoise / ptx_temporal_accumulate / ptx_denoise_variance since the last ptx_resize' are each
        read-back's refusal; 'ptx_resize drops the motion images'.  What the serials were is nobody's business without a history."""
        self.image = True
        self.bound = False
        self.guides = self.motion = self.temporal = self.moments = self.variance = False
        self.denoised_in = self.history_in = None
        return OK

    def scene_changed(self):
        """section 17: 'the upload and ptx_share_scene also forget the handle's own tags, which may stem from another owner's serials'
        and with them go the motion images, which led back to one of them"""
        self.guides_pose = self.temporal_pose = None
        self.motion = False

    def render_guides(self, motion=False):
        """'Refusals as ptx_render_guides', and PTX_ERROR_NOT_READY while the scene's owner does not track motion'; 'Every guide pass
        records the serial it rendered at'; 'a later plain ptx_render_guides makes them stale'"""
        if not self.usable or not self.image or self.bound or (motion and not self.pose.tracking):
            return NOT_READY
        self.motion_from = self.history_pose()
        self.guides, self.guides_pose, self.motion = True, self.pose.serial, motion
        return OK

    def ladder(self, motion=False):
        """the reasons every stage behind the guide pass shares, in the order they are reported"""
        if not self.image:
            return "no image"
        if self.bound:
            return "bound shard"
        if not self.guides:
            return "no guides"
        if motion and not self.motion_fresh():
            return "stale motion"
        if self.world > 1:
            return "shards"
        return None

    def accumulate(self, moments=False, reset=False, motion=False):
        """section 14: the two copies of the history alternate, a call reads the one the call before wrote (none: no history, or
        PTX_TEMPORAL_RESET); 'A plain ptx_temporal_accumulate DROPS the moment history: the next moments call restarts'; 'every accepted
        accumulate call (plain, moments or motion) tags its history with the serial of the guides it consumed'.
        Returns the reason of the refusal, or (source copy, destination copy, history used, moment history used)."""
        why = self.ladder(motion)
        if why:
            return why
        use = self.history_in is not None and not reset
        plan = (self.history_in, 1 if self.history_in == 0 else 0, use, use and self.moments)
        self.history_in, self.moments, self.temporal, self.temporal_pose = plan[1], moments, True, self.guides_pose
        return plan

    def denoise(self, iterations, source="image"):
        """section 13: iteration i writes image i & 1 of the two the filter alternates between, so D is where the last one wrote;
        ptx_denoise_temporal: 'Refusals as ptx_denoise's, and PTX_ERROR_NOT_READY: no ptx_temporal_accumulate since the last ptx_resize'"""
        if source == "temporal" and not self.temporal:
            return "no T"
        why = self.ladder()
        if why:
            return why
        self.denoised_in = (iterations - 1) & 1
        return None

    def denoise_variance(self, iterations):
        """'PTX_ERROR_NOT_READY: whatever ptx_denoise_temporal answers so, and unless the last accepted accumulate call since
        ptx_resize was ptx_temporal_accumulate_moments'; 'output: D where ptx_denoise leaves it ... and V_0 for ptx_read_variance'"""
        why = self.ladder() or (None if self.moments_current() else "moments")
        if why:
            return why
        self.denoised_in, self.variance = (iterations - 1) & 1, True
        return None


# =====================================================================================================
# without a GPU: the header alone
# =====================================================================================================

_PROGRAM = r"""
#include "pt_chain_state.hpp"
#include <cstdio>
// One sequence per line of stdin, one letter per event; after every event the whole status on a line of its own.  The scene's side
// (serial, snapshot) is kept here: Z resize, S scene change, P / p pose update with / without a snapshot, g / m plain / motion guide
// pass, a A b B accumulate (plain, plain RESET, moments, moments RESET), f F plain filter with 1 / 2 iterations, v V the variance
// filter.  An event whose precondition the status does not meet is answered "refused" and changes nothing.
static void pose(uint64_t p) { if (p == ChainStatus::kNoPose) printf(" -"); else printf(" %llu", (unsigned long long)p); }
int main()
{
    ChainStatus s;
    uint64_t serial = 0;
    bool snapshot = false;
    for (int ch; (ch = getchar()) != EOF;)
    {
        if (ch == '\n')
        {
            s = ChainStatus();
            serial = 0;
            snapshot = false;
            continue;
        }
        const bool moments = ch == 'b' || ch == 'B', reset = ch == 'A' || ch == 'B';
        char note[64] = "";
        switch (ch)
        {
        case 'Z': s.resize(); break;
        case 'S': s.sceneChanged(); serial += 2; snapshot = false; break;
        case 'P': serial++; snapshot = true; break;
        case 'p': serial++; snapshot = false; break;
        case 'g': s.guidesRendered(serial, false); break;
        case 'm':
        {
            const PrevPoseSource from = ChainStatus::prevPoseSource(s.historyPose(), serial, snapshot);
            snprintf(note, sizeof note, "%s", from == PrevPoseSource::kCurrent ? "current" : from == PrevPoseSource::kSnapshot ? "snapshot" : "unknown");
            s.guidesRendered(serial, true);
            break;
        }
        case 'a': case 'A': case 'b': case 'B':
            if (s.guidesReady)
            {
                const ChainStatus::Accumulate a = s.accumulate(moments, reset);
                snprintf(note, sizeof note, "%d %d %d %d", a.src, a.dst, (int)a.useHistory, (int)a.useMoments);
            }
            else
                snprintf(note, sizeof note, "refused");
            break;
        case 'f': case 'F':
            if (s.guidesReady) s.filtered(ch == 'f' ? 1u : 2u);
            else snprintf(note, sizeof note, "refused");
            break;
        case 'v': case 'V':
            if (s.guidesReady && s.momentsCurrent()) s.varianceFiltered(ch == 'v' ? 1u : 2u);
            else snprintf(note, sizeof note, "refused");
            break;
        default: return 2;
        }
        printf("%c %d %d %d %d %d %d %d", ch, (int)s.guidesReady, s.denoisedIn, (int)s.temporalReady, s.historyIn, (int)s.momentsLive, (int)s.varianceReady,
               (int)s.motionReady);
        pose(s.guidesPose); pose(s.temporalPose); pose(s.motionFromPose); pose(s.historyPose());
        printf(" %d %d | %s\n", (int)s.motionFresh(), (int)s.momentsCurrent(), note);
    }
    return 0;
}
"""

ALPHABET = "ZSPpgmaAbBfFvV"


def _model_lines(sequence):
    """what the program prints for one sequence, from the model"""
    m = Model()
    m.image = m.usable = True
    m.pose.tracking = True  # (a scene change stands for an upload with ptx_track_motion called again, or a ptx_share_scene)
    out = []
    for ch in sequence:
        note = ""
        if ch == "Z":
            m.resize()
        elif ch == "S":
            m.scene_changed()
            m.pose.upload()
            m.pose.tracking = True
        elif ch in "Pp":
            m.pose.tracking = ch == "P"
            m.pose.update()
            m.pose.tracking = True
        elif ch == "g":
            m.render_guides()
        elif ch == "m":
            note = m.prev_pose()
            m.render_guides(True)
        elif ch in "aAbB":
            plan = m.accumulate(moments=ch in "bB", reset=ch in "AB")
            note = "refused" if isinstance(plan, str) else "%d %d %d %d" % (-1 if plan[0] is None else plan[0], plan[1], plan[2], plan[3])
        elif ch in "fF":
            note = "refused" if m.denoise(1 if ch == "f" else 2) else ""
        else:
            note = "refused" if m.denoise_variance(1 if ch == "v" else 2) else ""
        p = lambda v: "-" if v is None else str(v)  # noqa: E731
        i = lambda v: -1 if v is None else v  # noqa: E731
        out.append("%s %d %d %d %d %d %d %d %s %s %s %s %d %d | %s" % (
            ch, m.guides, i(m.denoised_in), m.temporal, i(m.history_in), m.moments, m.variance, m.motion, p(m.guides_pose), p(m.temporal_pose),
            p(m.motion_from), p(m.history_pose()), m.motion_fresh(), m.moments_current(), note))
    return out


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_every_sequence_of_up_to_four_events_against_the_model(pkg, tmp_path, flags):
    """pt_chain_state.hpp compiles with the host compiler and nothing else, and after every event of every sequence the whole status,
    the three predicates, the copies an accumulate call reads and writes and the previous pose a motion pass takes are the model's."""
    src, exe = tmp_path / "chain.cpp", tmp_path / "chain"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(pkg.PKG_DIR, "csrc"), str(src), "-o", str(exe)])
    sequences = ["".join(s) for n in range(1, 5) for s in itertools.product(ALPHABET, repeat=n)]
    assert len(sequences) == 14 + 14 ** 2 + 14 ** 3 + 14 ** 4
    done = subprocess.run([str(exe)], input="".join(s + "\n" for s in sequences), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and not done.stderr, done.stderr[-2000:]
    got = done.stdout.split("\n")[:-1]
    assert len(got) == sum(len(s) for s in sequences)
    at = 0
    for s in sequences:
        want = _model_lines(s)
        assert got[at:at + len(s)] == want, (s, got[at:at + len(s)], want)
        at += len(s)


def test_the_header_has_no_hip_in_it(pkg):
    text = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_chain_state.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>"], includes
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert not re.search(r"hip|DevBuf|float4|\[16\]", code, re.I), "buffers, matrices and HIP belong to ChainState (pt_runtime.hpp)"


# =====================================================================================================
# on the GPU
# =====================================================================================================

TD = dict(max_history=8.0, normal_threshold=0.3, position_threshold=0.03)
RESET = 1  # PTX_TEMPORAL_RESET


class _Handle:
    """A renderer and its model side by side: every call goes to both, and the answers are compared"""

    def __init__(self, pkg, scene):
        self.pkg, self.scene, self.r, self.m = pkg, scene, pkg.Renderer(), Model()
        self.u = scene.uniform(W, H, bounces=2)
        self.cam = scene.camera_matrices(W, H)
        self.keep = []  # device buffers bound as shard accumulation
        self.shard_now = (1, 32)  # worldSize and tileSize of the last ptx_set_tile_shard
        self.borrows = False

    def close(self):
        self.r.close()

    def call(self, fn, *a, **k):
        """(status, message) of one call of the Python layer"""
        try:
            fn(*a, **k)
            return OK, ""
        except self.pkg.PtxError as e:
            code, text = re.match(r"status (\d+): (.*)", str(e), re.S).groups()
            return int(code), text

    def expect(self, want, got, what):
        assert got[0] == want, (what, want, got)
        self.check(what)

    def check(self, what):
        """the four device pointers and the two read-backs whose state no pointer shows"""
        r, m = self.r, self.m
        for k in range(3):
            assert bool(r.guide_ptr(k)) == m.guides, (what, "guide", k)
        for k in range(2):
            assert bool(r.motion_ptr(k)) == m.motion, (what, "motion", k)
        assert bool(r.temporal_ptr()) == m.temporal, (what, "T")
        assert bool(r.denoised_ptr()) == (m.denoised_in is not None), (what, "D")
        assert self.call(r.read_moments)[0] == (OK if m.moments_current() else NOT_READY), (what, "moments")
        assert self.call(r.read_variance)[0] == (OK if m.variance else NOT_READY), (what, "V_0")

    # ---- the calls ----
    def upload(self):
        """ptx_scene_upload and ptx_build_accel; a renderer that was borrowing a scene gets its own again"""
        if self.borrows:
            self.m.pose, self.borrows = PoseModel(), False
        self.m.pose.upload()
        self.m.scene_changed()
        self.m.usable = True
        self.expect(OK, self.call(self.r.upload, self.scene), "upload")

    def share(self, owner):
        self.m.pose, self.m.usable, self.borrows = owner.m.pose, True, True
        self.m.scene_changed()
        self.expect(OK, self.call(self.r.share_scene, owner.r), "share_scene")

    def resize(self):
        self.expect(self.m.resize(), self.call(self.r.resize, W, H), "resize")

    def shard(self, world, bind=False):
        """ptx_set_tile_shard, then with `bind` a shard accumulation buffer"""
        import torch

        new = (world, 8 if world > 1 else 32)
        if new != self.shard_now:  # 'the bound buffer was laid out for another shard'
            self.m.bound = False
        self.shard_now, self.m.world = new, world
        self.expect(OK, self.call(self.r.set_tile_shard, 0, *new), "set_tile_shard")
        if bind:
            n = self.r.shard_bytes(0)
            self.keep.append(torch.zeros(n // 4, dtype=torch.float32, device="cuda"))
            self.m.bound = True
            self.expect(OK, self.call(self.r.bind_shard_accumulation, self.keep[-1].data_ptr(), n), "bind_shard_accumulation")

    def track(self, enable):
        self.m.pose.track(enable)
        self.expect(OK, self.call(self.r.track_motion, enable), "track_motion")

    def pose(self, state):
        it, bn = state
        self.m.pose.update()
        self.expect(OK, self.call(self.r.update_animation, it, bn if bn is not None and len(bn) else None), "update_animation")

    def guides(self, motion=False):
        want = self.m.render_guides(motion)
        self.expect(want, self.call(self.r.render_guides_motion if motion else self.r.render_guides, self.u), "guides motion=%s" % motion)

    def accumulate(self, moments=False, reset=False, motion=False, samples=1, with_moments=None):
        """with_moments: the raw third argument of ptx_temporal_accumulate_motion"""
        flags = RESET if reset else 0
        if with_moments is not None or samples == 0:
            want = INVALID  # the arguments are looked at first: the model is not asked and nothing changes
        else:
            want = NOT_READY if isinstance(self.m.accumulate(moments, reset, motion), str) else OK
        if motion:
            got = self.call(self.r.temporal_accumulate_motion, samples, *self.cam, flags=flags, moments=moments if with_moments is None else with_moments, **TD)
        else:
            got = self.call(self.r.temporal_accumulate_moments if moments else self.r.temporal_accumulate, samples, *self.cam, flags=flags, **TD)
        self.expect(want, got, "accumulate moments=%s reset=%s motion=%s" % (moments, reset, motion))
        return got

    def denoise(self, iterations, source="image"):
        if source == "temporal" and not self.m.temporal:
            want = NOT_READY  # ptx_denoise_temporal asks for T before it hands the descriptor to ptx_denoise's checks
        else:
            want = INVALID if not 1 <= iterations <= 6 else NOT_READY if self.m.denoise(iterations, source) else OK
        got = self.call(self.r.denoise_temporal, iterations) if source == "temporal" else self.call(self.r.denoise, 1, iterations)
        self.expect(want, got, "denoise %d of %s" % (iterations, source))
        return got

    def variance(self, iterations):
        want = INVALID if not 1 <= iterations <= 6 else NOT_READY if self.m.denoise_variance(iterations) else OK
        got = self.call(self.r.denoise_variance, iterations)
        self.expect(want, got, "denoise_variance %d" % iterations)
        return got


@pytest.fixture(scope="module")
def owners(pkg):
    """Two scene owners, uploaded once: the `default` scene, and animated_test (tests/test_motion.py's, with its poses) for the
    sequences that update the pose"""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)
    import test_motion as TM

    animated = TM._case(pkg, "animated_test")
    made = []

    def make(which):
        h = _Handle(pkg, pkg.Scene("default") if which == "default" else animated.scene)
        h.upload()
        made.append(h)
        return h

    yield make("default"), make("animated"), animated.states
    for h in made:
        h.close()


def _borrower(pkg, owner, resize=True):
    b = _Handle(pkg, owner.scene)
    b.share(owner)
    if resize:
        b.resize()
    return b


def _plain_chain(pkg, default, animated, states):
    """every stage once, a second extent, and the first stages again"""
    b = _borrower(pkg, default, resize=False)
    b.guides(), b.accumulate(), b.denoise(1)  # no image yet: all refused
    b.resize()
    b.accumulate(), b.denoise(2), b.denoise(1, "temporal"), b.variance(1)  # no guides
    b.guides(), b.denoise(1, "temporal"), b.variance(1)  # no T, no moments
    b.accumulate(), b.denoise(2), b.denoise(1, "temporal"), b.variance(2)
    b.accumulate(moments=True), b.variance(2), b.variance(1)
    b.resize()
    b.denoise(1), b.accumulate(moments=True), b.variance(1)
    b.guides(), b.accumulate(moments=True), b.variance(1)
    return [b]


def _plain_after_moments(pkg, default, animated, states):
    b = _borrower(pkg, default)
    b.guides(), b.accumulate(moments=True), b.accumulate(moments=True), b.variance(3)
    b.accumulate()  # a plain call drops the moment history
    b.variance(1), b.denoise(2, "temporal")
    b.accumulate(moments=True), b.variance(1)
    return [b]


def _reset_flag(pkg, default, animated, states):
    b = _borrower(pkg, default)
    b.guides(), b.accumulate(moments=True, reset=True), b.accumulate(moments=True), b.accumulate(moments=True, reset=True), b.variance(1)
    b.accumulate(reset=True), b.variance(1)
    b.accumulate(moments=True, reset=True), b.variance(2)
    return [b]


def _bad_arguments(pkg, default, animated, states):
    """the arguments come first, whatever the state, and a refused call changes nothing"""
    b = _borrower(pkg, default)
    b.accumulate(motion=True, with_moments=2), b.accumulate(samples=0), b.denoise(0), b.denoise(7, "temporal"), b.variance(0)
    b.guides(), b.accumulate(moments=True), b.variance(1)
    b.accumulate(motion=True, with_moments=2), b.accumulate(samples=0), b.accumulate(moments=True, samples=0), b.denoise(7), b.denoise(7, "temporal"), b.variance(7)
    b.variance(2)
    return [b]


def _tile_shards(pkg, default, animated, states):
    b = _borrower(pkg, default)
    b.guides(), b.accumulate(moments=True)
    b.shard(2)
    b.guides(), b.accumulate(), b.accumulate(moments=True), b.denoise(1), b.denoise(1, "temporal"), b.variance(1)
    b.shard(2, bind=True)
    b.guides(), b.accumulate(), b.denoise(1), b.variance(1)
    b.shard(1)  # another shard: the binding goes, and the chain is where it was
    b.variance(1), b.accumulate(), b.denoise(2, "temporal")
    b.shard(1, bind=True)
    b.guides(), b.accumulate(), b.denoise(1, "temporal")
    b.resize()  # a new extent unbinds
    b.guides(), b.accumulate()
    return [b]


def _upload_on_an_owner(pkg, default, animated, states):
    """the guides and T outlive an upload; the motion images and the pose tags do not"""
    o = _Handle(pkg, animated.scene)
    o.upload(), o.resize(), o.track(True)
    o.guides(motion=True), o.accumulate(motion=True), o.guides(motion=True), o.accumulate(moments=True, motion=True)
    o.upload()
    o.accumulate(motion=True)  # stale
    o.guides(motion=True)  # the upload turned tracking off
    o.variance(1), o.accumulate(moments=True), o.track(True)
    o.guides(motion=True), o.accumulate(motion=True), o.accumulate(motion=True)  # the second one: the history moved to the new pose
    return [o]


def _share_scene_on_a_borrower(pkg, default, animated, states):
    animated.track(True)
    b = _borrower(pkg, animated)
    b.guides(motion=True), b.accumulate(motion=True), b.guides(motion=True)
    b.share(animated)
    b.accumulate(motion=True), b.accumulate(), b.guides(motion=True), b.accumulate(motion=True, moments=True), b.variance(1)
    b.share(default)  # nobody tracks there
    b.guides(motion=True), b.guides(), b.accumulate(motion=True), b.accumulate()
    return [b]


def _plain_guides_after_motion_guides(pkg, default, animated, states):
    animated.track(True)
    b = _borrower(pkg, animated)
    b.guides(motion=True), b.guides()
    b.accumulate(motion=True), b.accumulate(), b.guides(motion=True), b.accumulate(motion=True), b.accumulate(motion=True)
    return [b]


def _update_between_guides_and_accumulate(pkg, default, animated, states):
    animated.track(True)
    b = _borrower(pkg, animated)
    b.guides(motion=True), b.accumulate(motion=True), b.guides(motion=True)
    animated.pose(states[1])
    b.accumulate(motion=True)  # the motion guides still lead back to the history as it stands
    b.guides(motion=True), b.accumulate(motion=True, moments=True), b.accumulate(motion=True, moments=True)
    animated.pose(states[2]), animated.pose(states[0])
    b.guides(motion=True), b.accumulate(motion=True), b.variance(1)
    return [b]


def _tracking_switched(pkg, default, animated, states):
    animated.track(False)
    b = _borrower(pkg, animated)
    b.guides(motion=True), b.guides(), b.accumulate()
    animated.pose(states[1])
    animated.track(True)
    b.guides(motion=True), b.accumulate(motion=True)
    animated.track(False)
    b.guides(motion=True), b.accumulate(motion=True), b.accumulate(motion=True)
    animated.pose(states[0])
    return [b]


def _resize_with_everything_live(pkg, default, animated, states):
    animated.track(True)
    b = _borrower(pkg, animated)
    b.guides(motion=True), b.accumulate(motion=True, moments=True), b.variance(2)
    b.resize()
    b.accumulate(motion=True), b.denoise(1, "temporal"), b.variance(1)
    b.guides(motion=True), b.accumulate(motion=True), b.denoise(1)
    return [b]


def _owner_without_an_extent(pkg, default, animated, states):
    o = _Handle(pkg, default.scene)
    o.guides()  # no scene
    o.upload()
    o.guides(), o.accumulate(), o.resize(), o.guides(), o.accumulate(reset=True), o.denoise(3)
    return [o]


SEQUENCES = [_plain_chain, _plain_after_moments, _reset_flag, _bad_arguments, _tile_shards, _upload_on_an_owner, _share_scene_on_a_borrower,
             _plain_guides_after_motion_guides, _update_between_guides_and_accumulate, _tracking_switched, _resize_with_everything_live,
             _owner_without_an_extent]


@pytest.mark.gpu
@pytest.mark.parametrize("sequence", SEQUENCES, ids=lambda f: f.__name__.strip("_"))
def test_call_sequences_on_a_handle_follow_the_model(pkg, owners, sequence):
    """After every call: its code is the model's, ptx_device_guide_ptr, _motion_ptr, _temporal_ptr and _denoised_ptr are null exactly
    where the model has nothing, and ptx_read_moments and ptx_read_variance are refused exactly when it says so."""
    default, animated, states = owners
    for h in sequence(pkg, default, animated, states):
        h.close()


# ---- the refusal ladder, word for word ---------------------------------------------------------------------------------

ELSEWHERE = ("%s: the accumulation of this renderer lives in a shard buffer (ptx_bind_shard_accumulation); the frame is composed by "
             "ptx_unpack_shards on the rank that gathers it")
STALE = "%s: the motion guides are stale: a ptx_render_guides or an accumulate call came after the last ptx_render_guides_motion"
NO_T = "ptx_denoise_temporal: call ptx_temporal_accumulate first"
# per entry point: (the call on a _Handle, {reason: the message}); a reason that an entry point cannot be in is left out
ENTRY_POINTS = {
    "ptx_denoise": (lambda h: h.denoise(1), {
        "no image": "ptx_denoise: no accumulation image (call ptx_resize)",
        "bound shard": ELSEWHERE % "ptx_denoise",
        "no guides": "ptx_denoise: no guides for this extent (call ptx_render_guides)",
        "shards": "ptx_denoise: this renderer holds one tile shard of 2; the filter's taps cross tiles"}),
    "ptx_denoise_temporal": (lambda h: h.denoise(1, "temporal"), {  # without an image or guides there is no T either, which comes first
        "no T": NO_T,
        "bound shard": ELSEWHERE % "ptx_denoise_temporal",
        "shards": "ptx_denoise_temporal: this renderer holds one tile shard of 2; the filter's taps cross tiles"}),
    "ptx_temporal_accumulate": (lambda h: h.accumulate(), {
        "no image": "ptx_temporal_accumulate: no accumulation image (call ptx_resize)",
        "bound shard": ELSEWHERE % "ptx_temporal_accumulate",
        "no guides": "ptx_temporal_accumulate: no guides for this extent (call ptx_render_guides)",
        "shards": "ptx_temporal_accumulate: this renderer holds one tile shard of 2; the history's taps cross tiles"}),
    "ptx_temporal_accumulate_moments": (lambda h: h.accumulate(moments=True), {
        "no image": "ptx_temporal_accumulate_moments: no accumulation image (call ptx_resize)",
        "bound shard": ELSEWHERE % "ptx_temporal_accumulate_moments",
        "no guides": "ptx_temporal_accumulate_moments: no guides for this extent (call ptx_render_guides)",
        "shards": "ptx_temporal_accumulate_moments: this renderer holds one tile shard of 2; the history's taps cross tiles"}),
    "ptx_temporal_accumulate_motion": (lambda h: h.accumulate(motion=True), {
        "no image": "ptx_temporal_accumulate_motion: no accumulation image (call ptx_resize)",
        "bound shard": ELSEWHERE % "ptx_temporal_accumulate_motion",
        "no guides": "ptx_temporal_accumulate_motion: no guides for this extent (call ptx_render_guides)",
        "stale motion": STALE % "ptx_temporal_accumulate_motion",
        "shards": "ptx_temporal_accumulate_motion: this renderer holds one tile shard of 2; the history's taps cross tiles"}),
    "ptx_denoise_variance": (lambda h: h.variance(1), {
        "no image": "ptx_denoise_variance: no accumulation image (call ptx_resize)",
        "bound shard": ELSEWHERE % "ptx_denoise_variance",
        "no guides": "ptx_denoise_variance: no guides for this extent (call ptx_render_guides)",
        "shards": "ptx_denoise_variance: this renderer holds one tile shard of 2; the filter's taps cross tiles",
        "moments": "ptx_denoise_variance: the last accumulate call must be ptx_temporal_accumulate_moments"}),
}


def _no_image(b):
    pass


def _bound_shard(b):
    b.resize(), b.guides(motion=True), b.accumulate(moments=True, motion=True), b.shard(1, bind=True)


def _no_guides(b):
    b.resize()


def _stale_motion(b):
    b.resize(), b.guides(motion=True), b.accumulate(moments=True), b.guides()


def _two_shards(b):
    b.resize(), b.guides(motion=True), b.accumulate(moments=True, motion=True), b.guides(motion=True), b.shard(2)


def _moments_not_live(b):
    b.resize(), b.guides(motion=True), b.accumulate(motion=True), b.guides(motion=True), b.accumulate(motion=True)


def _no_guides_and_two_shards(b):
    b.resize(), b.shard(2)


def _stale_motion_and_two_shards(b):
    _stale_motion(b), b.shard(2)


def _bound_shard_and_no_guides(b):
    b.resize(), b.shard(2, bind=True)


# state -> the reason each entry point must report in it, in the ladder's order (None: the call is accepted)
LADDER = [
    (_no_image, lambda name: "no T" if name == "ptx_denoise_temporal" else "no image"),
    (_bound_shard, lambda name: "bound shard"),
    (_no_guides, lambda name: "no T" if name == "ptx_denoise_temporal" else "no guides"),
    (_stale_motion, lambda name: "stale motion" if name == "ptx_temporal_accumulate_motion" else None),
    (_two_shards, lambda name: "shards"),
    (_moments_not_live, lambda name: "moments" if name == "ptx_denoise_variance" else None),
    (_no_guides_and_two_shards, lambda name: "no T" if name == "ptx_denoise_temporal" else "no guides"),
    (_stale_motion_and_two_shards, lambda name: "stale motion" if name == "ptx_temporal_accumulate_motion" else "shards"),
    (_bound_shard_and_no_guides, lambda name: "no T" if name == "ptx_denoise_temporal" else "bound shard"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("state,reason", LADDER, ids=[s.__name__.strip("_") for s, _ in LADDER])
def test_refusals_of_the_shared_ladder_word_for_word(pkg, owners, state, reason):
    """A handle in each state of the ladder, alone and where two reasons hold at once: ptx_last_error after every refused chain entry
    point is the message written out above (the earlier reason's), with code 5; the refused calls are made first, so that they meet
    the state as it was built."""
    default, animated, states = owners
    animated.track(True)
    b = _borrower(pkg, animated, resize=False)
    try:
        state(b)
        for accepted in (False, True):
            for name, (call, messages) in ENTRY_POINTS.items():
                why = reason(name)
                if (why is None) != accepted:
                    continue
                got = call(b)  # (the code is compared with the model's inside)
                if why is None:
                    assert got == (OK, ""), (name, got)
                else:
                    assert got == (NOT_READY, messages[why]), (name, why, got)
    finally:
        b.close()
