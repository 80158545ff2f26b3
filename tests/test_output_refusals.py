"""What every entry point of the output stage answers in every state of the handle (csrc/pt_output_host.hpp; include/ptx.h:
ptx_postprocess*, ptx_meter, ptx_local_exposure, ptx_grade, ptx_present*, and their read-backs).

One 33 x 22 handle walks through the states of STATES, in that order.  In every state each call of CALLS is made through the raw
library, in that order, and the test holds the returned code against TABLE, written out below from the refusal paragraphs of
include/ptx.h, and the handle's last-error text of every refused call against that entry point's name.

The calls are real ones: an accepted call does what it does, so it moves the handle on within the row.  ptx_postprocess sets the
output ready for what follows it, the first accepted ptx_meter makes the meter's state, which outlives ptx_resize, the first accepted
ptx_local_exposure makes G.  The rows are therefore read with the walk in mind:

  a  nothing exists.  ptx_read_present's "nothing presented yet" is PTX_ERROR_INVALID_ARGUMENT, every other refusal is
     PTX_ERROR_NOT_READY
  b  the metered and the local output calls come before ptx_meter and ptx_local_exposure and are refused; C and D do not exist
  c  C exists, D does not
  d - g  everything exists and every call is accepted
  h  a tile shard of two: the meter, the local exposure, its output call and the grade refuse, the other output calls do not
  i  a bound shard buffer: whatever reads the sum refuses, and so do the grade and both presents; the output calls on C and D and
     the read-backs do not
  j  ptx_resize under the shard of h: the bound buffer, C, D, G and the ready output are gone, the meter's state, the kept grade desc
     and the present image are not
  k  the same with one shard again: ptx_postprocess_local misses G until ptx_local_exposure has run, ptx_present_graded finds the desc
     that ptx_grade left before the resize"""
import ctypes as C

import numpy as np
import pytest

W, H, SAMPLES = 33, 22, 4
OK, INVALID, NOT_READY = 0, 1, 5

# name of the entry point, and the arguments behind the handle
CALLS = (
    [("ptx_postprocess", ()), ("ptx_postprocess_despiked", ()), ("ptx_postprocess_denoised", ())]
    + [("ptx_postprocess_metered", (source,)) for source in (0, 1, 2)]
    + [("ptx_postprocess_local", (source, metered)) for source in (0, 1, 2) for metered in (0, 1)]
    + [("ptx_meter", (source,)) for source in (0, 1, 2)]
    + [("ptx_local_exposure", (source, pivot_metered)) for source in (0, 1, 2) for pivot_metered in (0, 1)]
    + [("ptx_grade", ()), ("ptx_present", ()), ("ptx_present_graded", ()), ("ptx_read_output", ()), ("ptx_read_present", ()), ("ptx_read_meter", ()),
       ("ptx_read_local_exposure", ())])

STATES = ("a: created, never resized", "b: resized, a few samples in the sum", "c: after ptx_despike", "d: after ptx_render_guides and ptx_denoise",
          "e: after ptx_meter", "f: after ptx_local_exposure", "g: after an output call", "h: set_tile_shard(0, 2, 8)",
          "i: a bound shard accumulation buffer", "j: a fresh ptx_resize, the shard of h still set", "k: one shard again and a fresh ptx_resize")

# one digit per call of CALLS: postprocess, _despiked, _denoised | metered 0 1 2 | local 00 01 10 11 20 21 | meter 0 1 2 |
# local_exposure 00 01 10 11 20 21 | grade, present, present_graded | read_output, read_present, read_meter, read_local_exposure
TABLE = {
    "a": "555 555 555555 555 555555 555 5155",
    "b": "055 555 555555 055 005555 000 0000",
    "c": "005 005 000055 005 000055 000 0000",
    "d": "000 000 000000 000 000000 000 0000",
    "e": "000 000 000000 000 000000 000 0000",
    "f": "000 000 000000 000 000000 000 0000",
    "g": "000 000 000000 000 000000 000 0000",
    "h": "000 000 555555 555 555555 505 0000",
    "i": "500 500 555555 555 555555 555 0000",
    "j": "055 055 555555 555 555555 505 0005",
    "k": "055 055 555555 055 005555 000 0000",
}


def _sum():
    rng = np.random.default_rng(33)
    S = np.empty((H, W, 4), np.float32)
    S[..., :3] = rng.uniform(0.0, 2.0 * SAMPLES, (H, W, 3))
    S[..., 3] = SAMPLES
    return S


@pytest.mark.gpu
def test_every_output_entry_point_in_every_state(pkg):
    import torch  # first, so the HIP library shares torch's HIP runtime

    lib = pkg.load_hip()
    scene = pkg.Scene("default", 0.25)
    r = pkg.Renderer()
    r.upload(scene)
    h = r.handle

    u = pkg.PostProcessingUniformData(SAMPLES, 1.25, 0.8, 0.35)
    md = pkg.METER_DEFAULTS
    ld = pkg.LOCAL_EXPOSURE_DEFAULTS
    gd = pkg.GRADE_DEFAULTS
    grade = pkg.GradeDesc((C.c_float * 9)(*gd["colour_matrix"]), (C.c_float * 3)(*gd["slope"]), (C.c_float * 3)(*gd["offset"]), (C.c_float * 3)(*gd["power"]),
                          gd["saturation"], gd["curve"], gd["white_point"], 0, 0)
    screen = pkg.PresentDesc(W, H, pkg.PRESENT_R16G16B16A16_SFLOAT, 0, None, 0, 0)
    out = np.empty((H, W, 4), np.float32)
    shown = np.empty((H, W, 4), np.uint16)
    gain = np.empty((H, W), np.float32)
    result = pkg.MeterResult()

    def meter_desc(source):
        return pkg.MeterDesc(source, md["mode"], SAMPLES, (C.c_uint32 * 4)(0, 0, 0, 0), md["low_permille"], md["high_permille"], md["key_log2"],
                             md["compensation"], md["min_log2_exposure"], md["max_log2_exposure"], md["speed_up"], md["speed_down"], 1.0 / 60, 0, 0)

    def local_desc(source, pivot_metered):
        return pkg.LocalExposureDesc(source, SAMPLES, ld["cell_shift"], ld["pivot_log2"], ld["highlight_contrast"], ld["shadow_contrast"], ld["max_stops"],
                                     pkg.LOCAL_EXPOSURE_PIVOT_METERED if pivot_metered else 0, 0)

    def call(name, args):
        if name in ("ptx_postprocess", "ptx_postprocess_despiked", "ptx_postprocess_denoised", "ptx_postprocess_metered", "ptx_postprocess_local"):
            return getattr(lib, name)(h, C.byref(u), 0, *args)
        if name == "ptx_meter":
            return lib.ptx_meter(h, C.byref(meter_desc(*args)))
        if name == "ptx_local_exposure":
            return lib.ptx_local_exposure(h, C.byref(local_desc(*args)))
        if name == "ptx_grade":
            return lib.ptx_grade(h, C.byref(grade), 0)
        if name in ("ptx_present", "ptx_present_graded"):
            return getattr(lib, name)(h, C.byref(screen))
        if name == "ptx_read_output":
            return lib.ptx_read_output(h, pkg.OUTPUT_RGBA32F, out.ctypes.data, out.nbytes)
        if name == "ptx_read_present":
            return lib.ptx_read_present(h, shown.ctypes.data, shown.nbytes)
        if name == "ptx_read_meter":
            return lib.ptx_read_meter(h, C.byref(result), None)
        assert name == "ptx_read_local_exposure"
        return lib.ptx_read_local_exposure(h, gain.ctypes.data, gain.nbytes)

    shard = []

    def bind_shard():
        shard.append(torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda"))
        r.bind_shard_accumulation(shard[0].data_ptr(), r.shard_bytes(0))

    def resized_with_samples():
        r.resize(W, H)
        r.write_accumulation(_sum())

    def denoised():
        r.render_guides(scene.uniform(W, H, bounces=4))
        r.denoise(SAMPLES, 2, 1.5, 0.3, 0.03)

    def one_shard_resized():
        r.set_tile_shard(0, 1, 8)
        resized_with_samples()

    enter = {"a": lambda: None, "b": resized_with_samples, "c": lambda: r.despike(radius=1, rank=2, gain=1.5, min_taps=3), "d": denoised,
             "e": lambda: r.meter(SAMPLES), "f": lambda: r.local_exposure(SAMPLES), "g": lambda: r.postprocess(SAMPLES), "h": lambda: r.set_tile_shard(0, 2, 8),
             "i": bind_shard, "j": resized_with_samples, "k": one_shard_resized}
    assert [s[0] for s in STATES] == list(TABLE) == list(enter)
    wrong = []
    for state in STATES:
        enter[state[0]]()
        want = [int(c) for c in TABLE[state[0]].replace(" ", "")]
        assert len(want) == len(CALLS)
        for (name, args), code in zip(CALLS, want):
            got = call(name, args)
            text = lib.ptx_last_error(h).decode()
            if got != code:
                wrong.append(f"{state}: {name}{args} returned {got}, the table says {code} ({text})")
            elif got != OK and not text.startswith(name + ":"):
                wrong.append(f"{state}: {name}{args} refused with another call's text: {text}")
    r.close()
    assert not wrong, "\n".join(wrong)
