"""Firefly suppression (include/ptx.h "Firefly suppression": ptx_despike, ptx_chain_use_despiked, ptx_postprocess_despiked;
csrc/pt_despike.hpp, docs/NEXT_ROWS.md section 20) against tests/firefly_ref.py.

Tolerance: none.  Every operation of the rule is specified in float32 and in its order -- a luminance of two multiplies, two adds and
one more multiply without contraction, comparisons, one multiply by the gain, the project's specified reciprocal and four more
multiplies -- so the device's C equals the float32 reference bit for bit on the device's own read-back sum, NaN payloads included.
Extents: 1 x 1, 3 x 2 (smaller than either window), 5 x 3, 33 x 9 (one pixel into a second 32 x 8 tile on both axes), 67 x 45 and
300 x 200."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import denoise_ref as R
import firefly_ref as FR

DETAIL = 0.25
SCENE = "texture_test"
EXTENTS = {"1x1": (1, 1), "3x2": (3, 2), "5x3": (5, 3), "33x9": (33, 9), "67x45": (67, 45), "300x200": (300, 200)}
W, H = EXTENTS["67x45"]
POST = dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=0.35)
TD = dict(max_history=8.0, normal_threshold=0.3, position_threshold=0.03)
OK, INVALID, NOT_READY = 0, 1, 5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _window_size(radius):
    return (2 * radius + 1) ** 2 - 1


def _configs():
    """radius {1, 2} x rank {1, 2, 4} x gain {1, 1.5} x two minTaps: the smallest the call takes and all of the window but three"""
    for radius, rank, gain in itertools.product((1, 2), (1, 2, 4), (1.0, 1.5)):
        for min_taps in (rank, _window_size(radius) - 3):
            yield dict(radius=radius, rank=rank, gain=gain, min_taps=min_taps)


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_firefly_suppression(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_despike": r"PTX_API int ptx_despike\(PtxRenderer \*r, const PtxDespikeDesc \*desc\);",
        "ptx_read_despiked": r"PTX_API int ptx_read_despiked\(PtxRenderer \*r, void \*host, size_t bytes\);",
        "ptx_device_despiked_ptr": r"PTX_API void \*ptx_device_despiked_ptr\(PtxRenderer \*r\);",
        "ptx_chain_use_despiked": r"PTX_API int ptx_chain_use_despiked\(PtxRenderer \*r, int enable\);",
        "ptx_postprocess_despiked": r"PTX_API int ptx_postprocess_despiked\(PtxRenderer \*r, const PtxPostProcessingUniformData \*uniform, uint32_t toneMappingMode\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert re.search(r"typedef struct PtxDespikeDesc \{\s*uint32_t radius;[^}]*uint32_t rank;[^}]*uint32_t minTaps;[^}]*float\s+gain;[^}]*uint32_t flags;[^}]*"
                     r"uint32_t reserved;[^}]*\} PtxDespikeDesc;", header)
    D = pkg.DespikeDesc
    assert C.sizeof(D) == 24 and [getattr(D, f).offset for f in ("radius", "rank", "minTaps", "gain", "flags", "reserved")] == [0, 4, 8, 12, 16, 20]
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("Firefly suppression", "section 20", "IN THE SUM'S SCALE", "S is never written", "(0.2126f S(p).r + 0.7152f S(p).g) + 0.0722f S(p).b",
                   "COUNTS iff Y(p) is finite", "without p itself", "rank-th largest Y", "equal values counted separately", "b = +0 otherwise",
                   "n >= minTaps", "Y(p) >= 2^-126", "Y(p) > b", "s = b rcp(Y(p))", "C(p).a = S(p).a", "C(p) = S(p) bit for bit",
                   "A refused call leaves the previous C", "ptx_resize drops C", "sticky switch", "one last", "the caller's TotalSamples",
                   "a one-pixel emitter or sun is clamped", "energy is lost by design", "there is no guide term"):
        assert phrase in header, phrase
    for method in ("despike", "read_despiked", "despiked_ptr", "chain_use_despiked", "postprocess_despiked"):
        assert callable(getattr(pkg.Renderer, method))
    d = pkg.DESPIKE_DEFAULTS
    assert set(d) == {"radius", "rank", "gain", "min_taps"} and d["radius"] in (1, 2) and 1 <= d["rank"] <= 4 and d["gain"] >= 1
    assert d["rank"] <= d["min_taps"] <= _window_size(d["radius"])
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct FireflySettings\s*\{\s*bool Enabled = false;\s*uint32_t Radius = (\d+);\s*uint32_t Rank = (\d+);\s*float Gain = ([0-9.]+)f;\s*"
                  r"uint32_t MinTaps = (\d+);\s*\};", host)
    assert m and (int(m[1]), int(m[2]), float(m[3]), int(m[4])) == (d["radius"], d["rank"], d["gain"], d["min_taps"])
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    for call in ("ptx_despike(s_Renderer", "ptx_postprocess_despiked(s_Renderer", "ptx_chain_use_despiked(s_Renderer, 1)", "ptx_chain_use_despiked(s_Renderer, 0)"):
        assert call in adapter, call
    assert "--despike" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()
    state = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_chain_state.hpp")).read()
    assert "despikedReady" in state and "useDespiked" in state
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_despike.hpp")).read()
    assert "k_despike" in kernel and "__shared__ float lum" in kernel
    assert os.path.exists(os.path.join(pkg.REPO_DIR, "tools", "firefly_quality.py"))


def _const(h, w, value, alpha=3.0):
    S = np.empty((h, w, 4), np.float32)
    S[..., 0:3] = value
    S[..., 3] = alpha
    return S


DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64])


@DTYPES
def test_a_constant_image_comes_back_and_scaling_by_a_power_of_two_commutes(dtype):
    S = _const(9, 11, (0.3, 0.7, 0.1))
    for p in _configs():
        Cc, dec = FR.despike(S, dtype=dtype, **p)
        assert not dec["clamped"].any(), p
        if dtype is np.float32:
            assert (_bits(Cc) == _bits(S)).all(), p
    rng = np.random.default_rng(3)
    S = (rng.random((12, 17, 4)) ** 6 * 40).astype(np.float32)  # a long tail: plenty is clamped
    for p in _configs():
        a, da = FR.despike(S, dtype=dtype, **p)
        b, db = FR.despike(S * np.float32(2.0 ** 7), dtype=dtype, **p)
        assert (da["clamped"] == db["clamped"]).all() and da["clamped"].any(), p
        assert (a * dtype(2.0 ** 7) == b).all(), p  # bit for bit: a power of two moves exponents only


@DTYPES
def test_black_neighbours_zero_the_pixel_and_adjacent_spikes_protect_each_other_only_at_rank_1(dtype):
    S = _const(7, 7, 0.0)
    S[3, 3, 0:3] = (5.0, 2.0, 1.0)
    Cc, dec = FR.despike(S, 1, 1, 1, 1.0, dtype)
    assert dec["clamped"].sum() == 1 and dec["clamped"][3, 3] and (Cc[3, 3, 0:3] == 0).all() and Cc[3, 3, 3] == 3.0
    S = _const(7, 9, 1.0)
    S[3, 3, 0:3] = S[3, 4, 0:3] = 50.0
    for radius in (1, 2):
        Cc, dec = FR.despike(S, radius, 1, 1, 1.0, dtype)
        assert not dec["clamped"].any()  # each is the other's largest neighbour
        Cc, dec = FR.despike(S, radius, 2, 2, 1.0, dtype)
        assert dec["clamped"].sum() == 2 and dec["clamped"][3, 3] and dec["clamped"][3, 4]
        assert np.allclose(Cc[3, 3:5, 0:3], 1.0, rtol=2e-7, atol=0)


@DTYPES
def test_one_spike_becomes_the_gain_and_no_other_pixel_moves(dtype):
    S = _const(9, 9, 1.0)
    S[4, 4, 0:3] = 100.0
    for p in _configs():
        Cc, dec = FR.despike(S, dtype=dtype, **p)
        only = np.zeros((9, 9), bool)
        only[4, 4] = True
        assert (dec["clamped"] == only).all(), p
        assert np.allclose(Cc[4, 4, 0:3], p["gain"], rtol=4e-7, atol=0) and Cc[4, 4, 3] == 3.0
        moved = (Cc != S.astype(dtype)).any(axis=-1)
        assert (moved == only).all(), p


@DTYPES
def test_a_corner_has_3_or_8_neighbours(dtype):
    S = _const(6, 6, 1.0)
    S[0, 0, 0:3] = 9.0
    for radius, n in ((1, 3), (2, 8)):
        Cc, dec = FR.despike(S, radius, 1, n, 1.0, dtype)
        assert dec["n"][0, 0] == n and dec["clamped"][0, 0] and dec["n"][3, 3] == _window_size(radius)
        Cc, dec = FR.despike(S, radius, 1, n + 1, 1.0, dtype)
        assert not dec["clamped"].any() and (Cc[0, 0, 0:3] == 9.0).all()
    Cc, dec = FR.despike(_const(1, 1, 4.0), 2, 1, 1, 1.0, dtype)  # a pixel outside the image is in no window
    assert dec["n"][0, 0] == 0 and not dec["clamped"].any()


def test_non_finite_pixels_are_in_no_window_and_pass_through():
    S = _const(7, 7, 1.0)
    S[3, 3, 0:3] = 50.0
    S[3, 4, 1] = np.inf   # the spike's only brighter neighbour
    S[1, 1, 2] = np.nan
    S[5, 5, 0:3] = (np.inf, -np.inf, 0.0)  # Y is a NaN
    S[5, 1, 0] = -np.inf
    S.view(np.uint32)[1, 1, 2] = 0x7FC12345  # a payload to carry through
    for dtype in (np.float32, np.float64):
        Cc, dec = FR.despike(S, 1, 1, 1, 1.0, dtype)
        assert not dec["counts"][3, 4] and not dec["counts"][1, 1] and not dec["counts"][5, 5] and not dec["counts"][5, 1]
        assert dec["n"][3, 3] == 7 and dec["n"][2, 2] == 7 and dec["n"][0, 0] == 2
        assert dec["clamped"].sum() == 1 and dec["clamped"][3, 3] and np.allclose(Cc[3, 3, 0:3], 1.0, rtol=2e-7)
    Cc, _ = FR.despike(S, 1, 1, 1, 1.0, np.float32)
    keep = np.ones((7, 7), bool)
    keep[3, 3] = False
    assert (_bits(Cc)[keep] == _bits(S)[keep]).all()


@DTYPES
def test_denormal_luminance_negative_neighbours_and_alpha(dtype):
    S = _const(5, 5, 0.0, alpha=7.0)
    S[2, 2, 0:3] = np.float32(1e-39)  # Y is below 2^-126: left alone although every neighbour is black
    Cc, dec = FR.despike(S, 1, 1, 1, 1.0, dtype)
    assert dec["counts"][2, 2] and dec["above"][2, 2] and not dec["normal"][2, 2] and not dec["clamped"].any()
    S[2, 2, 0:3] = np.float32(2.0 ** -120)  # a small normal number is clamped
    Cc, dec = FR.despike(S, 1, 1, 1, 1.0, dtype)
    assert dec["clamped"][2, 2] and (Cc[2, 2, 0:3] == 0).all()
    S = _const(5, 5, -2.0, alpha=7.0)
    S[2, 2, 0:3] = (3.0, 1.0, 0.5)
    S[..., 3] = np.arange(25, dtype=np.float32).reshape(5, 5)
    Cc, dec = FR.despike(S, 2, 4, 8, 1.5, dtype)
    assert (dec["h"] < 0)[2, 2] and dec["b"][2, 2] == 0 and not np.signbit(dec["b"][2, 2])
    assert dec["clamped"].sum() == 1 and (Cc[2, 2, 0:3] == 0).all() and not np.signbit(Cc[2, 2, 0:3]).any()
    assert (Cc[..., 3] == S[..., 3]).all()  # alpha passes through, clamped or not


def test_the_specified_reciprocal():
    y = np.float32([2.0 ** -126, 2.0 ** 126, 3.0, -3.0, 1e-39, -1e-39, 0.0, 2.0 ** 127, -(2.0 ** 127)])
    r = FR.rcp(y)
    assert r[0] == np.float32(2.0 ** 126) and r[1] == np.float32(2.0 ** -126) and r[2] == np.float32(1.0) / np.float32(3.0) and r[3] == -r[2]
    assert r[4] == np.inf and r[5] == -np.inf and r[6] == np.inf and r[7] == 0 and not np.signbit(r[7]) and r[8] == 0 and np.signbit(r[8])


_quality = {}


def _quality_cases(pkg, orc):
    """tools/denoise_quality.py's 4-spp renders, truth and guides, once"""
    if not _quality:
        import sys
        sys.path.insert(0, os.path.join(pkg.REPO_DIR, "tools"))
        import denoise_quality as DQ
        truth = {k: v.astype(np.float32) for k, v in np.load(DQ.TRUTH).items()}
        for name in DQ.SCENES:
            s = pkg.Scene(name, DQ.DETAIL)
            _quality[name] = (DQ.render_sum(orc, s, DQ.LOW_SPP), truth[name], R.cpu_guides(pkg, orc, s, DQ.W, DQ.H), DQ.LOW_SPP)
    return _quality


def test_quality_relations_at_the_defaults(pkg, orc):
    """At DESPIKE_DEFAULTS, 4 spp against tests/golden/denoise_truth_512spp.npz: despiked < raw on all three scenes; despiked + filter <
    filter alone (DENOISE_DEFAULTS) on texture_test and alpha_test; `default` behind the filter is reported only."""
    p, dd = pkg.DESPIKE_DEFAULTS, pkg.DENOISE_DEFAULTS
    for name, (S, truth, guides, spp) in _quality_cases(pkg, orc).items():
        Cc, dec = FR.despike(S, **p)
        flt = lambda img: R.denoise(img, *guides, spp, dd["iterations"], dd["sigma_color"], dd["sigma_normal"], dd["sigma_position"], np.float32)  # noqa: E731
        raw, des = R.relative_l2(S[..., 0:3] / spp, truth), R.relative_l2(Cc[..., 0:3] / spp, truth)
        behind, both = R.relative_l2(flt(S), truth), R.relative_l2(flt(Cc), truth)
        print(f"{name}: raw {raw:.4f} -> despiked {des:.4f}; filter {behind:.4f} -> despiked + filter {both:.4f}; clamped {100 * dec['clamped'].mean():.1f} %")
        assert des < raw, name
        if name != "default":
            assert both < behind, name


# =====================================================================================================
# on the GPU
# =====================================================================================================
_state = {}


def _gpu(pkg):
    """(scene, renderer) of SCENE, uploaded once"""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if "main" not in _state:
        s = pkg.Scene(SCENE, DETAIL)
        r = pkg.Renderer()
        r.upload(s)
        _state["main"] = (s, r)
    return _state["main"]


def _synthetic_sum(h, w, seed=11):
    """A sum with everything the rule has a clause for.  Positions wrap, so every extent gets what fits."""
    rng = np.random.default_rng(seed)
    S = (rng.random((h, w, 4)) * 2).astype(np.float32)
    S[..., 3] = 2.0
    S[h // 2:, : max(1, w // 3), 0:3] = 1.0                     # ties
    S[: max(1, h // 3), w // 2:, 0:3] *= -1.0                   # negative values
    S[h // 3: h // 3 + 3, 0:3, 0:3] = np.float32(1e-41)         # denormals among denormals ...
    S[(h // 3 + 1) % h, 1 % w, 0:3] = np.float32(1e-39)         # ... and a spike among them that is no normal number

    def put(y, x, rgb):
        S[y % h, x % w, 0:3] = rgb
    put(2, 3, (np.nan, 1.0, 1.0))
    put(4, 5, (1.0, np.inf, 1.0))
    put(6, 2, (np.inf, -np.inf, 0.0))
    put(8, 9, (-np.inf, 0.0, 0.0))
    put(5, 12, 1e4)                                             # a hot pixel alone
    put(4, 6, 3e3)                                              # ... and one whose neighbour is an Inf
    put(10, 20, 5e3)
    put(10, 21, 5e3)                                            # an adjacent pair, equal
    put(20, 30, 4e3)
    put(21, 31, 6e3)                                            # ... and a diagonal one, unequal
    put(15, 40, 1e38)                                           # above 2^126: the reciprocal is zero
    put(15, 41, 3e37)
    put(16, 40, 9e37)
    put(30, 50, 1e-30)
    S.view(np.uint32)[2 % h, 3 % w, 0] = 0x7FC0BEEF
    return S


_sums = {}


def _sum(pkg, extent, kind):
    """The device's own read-back sum of `kind` at `extent` (render1, render8, synthetic) and the uniform it was rendered with"""
    key = (extent, kind)
    if key not in _sums:
        s, r = _gpu(pkg)
        w, h = EXTENTS[extent]
        r.set_tile_shard(0, 1, 32)
        r.resize(w, h)
        u = s.uniform(w, h, bounces=4)
        if kind == "synthetic":
            r.write_accumulation(_synthetic_sum(h, w))
        else:
            for f in range(int(kind[6:])):
                u.TotalSamples = f
                r.render(u, s.lights)
        _sums[key] = (r.readback(), s.uniform(w, h, bounces=4))
    return _sums[key]


def _plain(pkg, w, h, S=None):
    """a handle with no scene: ptx_despike needs none"""
    f = pkg.Renderer()
    f.resize(w, h)
    if S is not None:
        f.write_accumulation(S)
    return f


def _borrower(pkg, w, h, S=None, u=None):
    b = pkg.Renderer()
    b.share_scene(_gpu(pkg)[1])
    b.resize(w, h)
    if S is not None:
        b.write_accumulation(S)
    if u is not None:
        b.render_guides(u)
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["render1", "render8", "synthetic"])
@pytest.mark.parametrize("extent", list(EXTENTS))
def test_despiked_image_equals_the_float32_reference_bit_for_bit(pkg, extent, kind):
    S, _ = _sum(pkg, extent, kind)
    w, h = EXTENTS[extent]
    r = _plain(pkg, w, h, S)
    clamped = 0
    for p in _configs():
        r.despike(**p)
        got = r.read_despiked()
        want, dec = FR.despike(S, **p)
        differ = (_bits(got) != _bits(want)).any(axis=-1)
        if differ.any():
            y, x = np.argwhere(differ)[0]
            print(f"{extent} {kind} {p}: {int(differ.sum())} pixels differ, first ({x}, {y}): S {S[y, x]} got {got[y, x]} want {want[y, x]} "
                  f"n {dec['n'][y, x]} h {dec['h'][y, x]} clamped {dec['clamped'][y, x]}")
        assert not differ.any(), (extent, kind, p)
        clamped += int(dec["clamped"].sum())
    print(f"{extent} {kind}: {clamped} clamp decisions over {len(list(_configs()))} configurations")
    if w * h >= 15:
        assert clamped > 0
    assert (_bits(r.readback()) == _bits(S)).all()  # S is never written
    r.close()


@pytest.mark.gpu
def test_nothing_else_is_touched_and_two_calls_in_a_row_match_fresh_handles(pkg):
    s, main = _gpu(pkg)
    S, u = _sum(pkg, "67x45", "render1")
    r = _borrower(pkg, W, H, S, u)
    guides = [r.read_guide(k) for k in range(3)]
    calls = (dict(radius=2, rank=4, gain=1.0, min_taps=8), dict(radius=1, rank=1, gain=1.5, min_taps=3), dict(radius=2, rank=2, gain=1.0, min_taps=21))
    for p in calls:
        r.despike(**p)
        f = _plain(pkg, W, H, S)
        f.despike(**p)
        assert (_bits(r.read_despiked()) == _bits(f.read_despiked())).all(), p
        f.close()
    assert r.despiked_ptr() and (_bits(r.readback()) == _bits(S)).all()
    for k in range(3):
        assert (_bits(r.read_guide(k)) == _bits(guides[k])).all()
    r.close()
    # the next ptx_render continues the sum as if nothing had happened, and does not refresh C
    main.set_tile_shard(0, 1, 32)
    main.resize(W, H)
    up = s.uniform(W, H, bounces=4)

    def path_traced(n, between=None):
        main.reset()
        for k in range(n):
            if between and k == n - 1:
                between()
            up.TotalSamples = k
            main.render(up, s.lights)
        return main.readback()
    two = path_traced(2)
    again = path_traced(2, between=lambda: main.despike())
    assert (_bits(two) == _bits(again)).all()
    one = path_traced(1)
    assert (_bits(main.read_despiked()) == _bits(FR.despike(one, **pkg.DESPIKE_DEFAULTS)[0])).all()  # of the sum as it stood when the call was made


@pytest.mark.gpu
def test_the_switch_puts_the_despiked_image_in_the_sums_place(pkg):
    S, u = _sum(pkg, "67x45", "render1")
    s, _ = _gpu(pkg)
    view, proj = s.camera_matrices(W, H)
    r = _borrower(pkg, W, H, S, u)
    r.despike()
    Cc = r.read_despiked()
    assert (_bits(Cc) != _bits(S)).any()
    r.chain_use_despiked(True)
    f = _borrower(pkg, W, H, Cc, u)  # a handle whose sum is C

    def sequence(h, flags=0):
        out = []
        h.temporal_accumulate(1, view, proj, flags=flags, **TD)
        out.append(h.read_temporal())
        h.temporal_accumulate_responsive(1, view, proj, flags=flags, fast_history=2.0, clamp_sigma=1.5, responsive_flags=pkg.RESPONSIVE_MOMENTS, **TD)
        out += [h.read_temporal(), h.read_moments()]
        h.denoise(1, 3, 1.5, 0.3, 0.03)
        out.append(h.read_denoised())
        return out
    on, want = sequence(r), sequence(f)
    for k, (a, b) in enumerate(zip(on, want)):
        assert (_bits(a) == _bits(b)).all(), k
    assert (on[1][..., 3] > 1).any()  # the second call had a history
    f.close()
    # off again: the bits of a handle that never heard of the switch (PTX_TEMPORAL_RESET: r's history is the despiked one)
    r.chain_use_despiked(False)
    g = _borrower(pkg, W, H, S, u)
    off, untouched = sequence(r, flags=1), sequence(g, flags=1)
    for k, (a, b) in enumerate(zip(off, untouched)):
        assert (_bits(a) == _bits(b)).all(), k
    assert (_bits(off[0]) != _bits(on[0])).any()
    assert (_bits(r.read_despiked()) == _bits(Cc)).all() and (_bits(r.readback()) == _bits(S)).all()
    g.close()
    r.close()


@pytest.mark.gpu
def test_despiked_output_stage_and_present(pkg):
    S, _ = _sum(pkg, "67x45", "synthetic")
    r = _plain(pkg, W, H, S)
    r.despike(radius=1, rank=2, gain=1.5, min_taps=3)
    Cc = r.read_despiked()
    f = _plain(pkg, W, H, Cc)
    for tone in (pkg.TONE_MAPPING_SDR, pkg.TONE_MAPPING_HDR):
        r.postprocess_despiked(2, tone_mapping=tone, **POST)  # C is in the sum's scale: the caller's TotalSamples
        f.postprocess(2, tone_mapping=tone, **POST)
        for fmt in (pkg.OUTPUT_RGBA8_SRGB, pkg.OUTPUT_RGBA32F):
            a, b = r.read_output(fmt), f.read_output(fmt)
            assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), (tone, fmt)
        for sw, sh, fmt, mode in ((W, H, pkg.PRESENT_R8G8B8A8_SRGB, 0), (100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 0), (134, 90, pkg.PRESENT_A2B10G10R10_UNORM, 1)):
            r.present(sw, sh, fmt, mode)
            f.present(sw, sh, fmt, mode)
            assert (r.read_present().view(np.uint8) == f.read_present().view(np.uint8)).all(), (tone, sw, sh, fmt)
    f.close()
    # the plain output stage still reads the sum
    r.postprocess(2, **POST)
    f = _plain(pkg, W, H, S)
    f.postprocess(2, **POST)
    assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) == _bits(f.read_output(pkg.OUTPUT_RGBA32F))).all()
    f.close()
    r.close()


@pytest.mark.gpu
def test_a_borrower_a_bound_image_and_resize(pkg):
    import torch

    s, _ = _gpu(pkg)
    w, h = EXTENTS["33x9"]
    b = _borrower(pkg, w, h)
    u = s.uniform(w, h, bounces=4)
    b.render(u, s.lights)
    S = b.readback()
    p = dict(radius=2, rank=2, gain=1.0, min_taps=8)
    b.despike(**p)
    assert (_bits(b.read_despiked()) == _bits(FR.despike(S, **p)[0])).all()
    # a bound image is the sum
    bound = torch.from_numpy(_synthetic_sum(h, w, seed=5)).cuda()
    b.bind_accumulation(bound.data_ptr(), bound.numel() * 4)
    b.despike(**p)
    assert (_bits(b.read_despiked()) == _bits(FR.despike(bound.cpu().numpy(), **p)[0])).all()
    b.bind_accumulation(0, 0)
    # ptx_resize drops C; the switch survives it
    b.chain_use_despiked(True)
    b.resize(W, H)
    buf = np.zeros((H, W, 4), np.float32)
    post = pkg.PostProcessingUniformData(1, 1.0, 1.0, 1.0)
    assert b.lib.ptx_read_despiked(b.handle, buf.ctypes.data, buf.nbytes) == NOT_READY and not b.despiked_ptr()
    assert b.lib.ptx_postprocess_despiked(b.handle, C.byref(post), 0) == NOT_READY
    S67, u67 = _sum(pkg, "67x45", "render8")
    b.write_accumulation(S67)
    b.render_guides(u67)
    view, proj = s.camera_matrices(W, H)
    with pytest.raises(pkg.PtxError, match="ptx_despike"):
        b.temporal_accumulate(8, view, proj, **TD)  # the last rung: the switch is still on and there is no C
    assert not b.temporal_ptr()
    b.despike(**p)
    b.temporal_accumulate(8, view, proj, **TD)
    f = _borrower(pkg, W, H, FR.despike(S67, **p)[0], u67)
    f.temporal_accumulate(8, view, proj, **TD)
    assert (_bits(b.read_temporal()) == _bits(f.read_temporal())).all()
    f.close()
    b.close()


@pytest.mark.gpu
def test_refusals_leave_everything_intact(pkg):
    import torch

    s, _ = _gpu(pkg)
    S, u = _sum(pkg, "67x45", "render1")
    r = pkg.Renderer()  # an owner of its own: tile shards and bound buffers are refused on it
    r.upload(s)
    r.resize(W, H)
    r.write_accumulation(S)
    r.render_guides(u)
    lib = r.lib
    view, proj = s.camera_matrices(W, H)
    r.despike()
    r.chain_use_despiked(True)
    r.temporal_accumulate(1, view, proj, **TD)
    r.denoise(1, 2, 1.5, 0.3, 0.03)
    Cc, T, D = r.read_despiked(), r.read_temporal(), r.read_denoised()

    def intact():
        assert (_bits(r.read_despiked()) == _bits(Cc)).all() and (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.read_denoised()) == _bits(D)).all()

    def call(radius=2, rank=2, min_taps=8, gain=1.0, flags=0, reserved=0, handle=r.handle):
        d = pkg.DespikeDesc(radius, rank, min_taps, gain, flags, reserved)
        return lib.ptx_despike(handle, C.byref(d))

    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=0), dict(radius=3), dict(rank=0), dict(rank=5), dict(rank=3, min_taps=2), dict(min_taps=25), dict(radius=1, min_taps=9),
                dict(gain=0.99), dict(gain=-2.0), dict(gain=nan), dict(gain=inf), dict(flags=1), dict(reserved=1)):
        assert call(**bad) == INVALID, bad
    assert lib.ptx_despike(r.handle, None) == INVALID and call(handle=None) == INVALID
    assert lib.ptx_chain_use_despiked(None, 1) == INVALID
    buf = np.zeros((H, W, 4), np.float32)
    assert lib.ptx_read_despiked(r.handle, None, buf.nbytes) == INVALID
    assert lib.ptx_read_despiked(r.handle, buf.ctypes.data, buf.nbytes + 16) == INVALID and lib.ptx_read_despiked(r.handle, buf.ctypes.data, buf.nbytes - 16) == INVALID
    assert not buf.any()
    post = pkg.PostProcessingUniformData(1, 1.0, 1.0, 1.0)
    assert lib.ptx_postprocess_despiked(r.handle, None, 0) == INVALID and lib.ptx_postprocess_despiked(r.handle, C.byref(post), 2) == INVALID
    assert lib.ptx_postprocess_despiked(None, C.byref(post), 0) == INVALID
    intact()
    # a tile shard of a larger world, a bound shard buffer
    r.set_tile_shard(0, 2, 8)
    assert call() == NOT_READY
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert call() == NOT_READY
    r.bind_shard_accumulation(0)
    r.set_tile_shard(0, 1, 32)
    intact()
    # no image; no C
    fresh = pkg.Renderer()
    assert call(handle=fresh.handle) == NOT_READY
    assert lib.ptx_read_despiked(fresh.handle, buf.ctypes.data, buf.nbytes) == NOT_READY and not lib.ptx_device_despiked_ptr(fresh.handle)
    assert lib.ptx_postprocess_despiked(fresh.handle, C.byref(post), 0) == NOT_READY
    fresh.share_scene(r)
    fresh.resize(W, H)
    assert lib.ptx_read_despiked(fresh.handle, buf.ctypes.data, buf.nbytes) == NOT_READY and not lib.ptx_device_despiked_ptr(fresh.handle)
    assert lib.ptx_postprocess_despiked(fresh.handle, C.byref(post), 0) == NOT_READY
    # the last rung stands behind every other one: without guides that is the reason, with them the missing C
    fresh.chain_use_despiked(True)
    fresh.write_accumulation(S)
    with pytest.raises(pkg.PtxError, match="ptx_render_guides"):
        fresh.denoise(1, 2, 1.5, 0.3, 0.03)
    fresh.render_guides(u)
    with pytest.raises(pkg.PtxError, match="ptx_despike"):
        fresh.denoise(1, 2, 1.5, 0.3, 0.03)
    with pytest.raises(pkg.PtxError, match="ptx_despike"):
        fresh.temporal_accumulate_moments(1, view, proj, **TD)
    assert not fresh.denoised_ptr() and not fresh.temporal_ptr()
    fresh.chain_use_despiked(False)
    fresh.denoise(1, 2, 1.5, 0.3, 0.03)  # off: the call is what it was
    fresh.close()
    intact()
    r.close()


@pytest.mark.gpu
def test_renderer_hip_with_firefly_settings_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with FireflySettings on: two frames of
    animated_test through RendererHip with the denoiser, the temporal settings and motion vectors.  The sum, T and the output image of
    both frames equal ptx_despike at the adapter's defaults, ptx_chain_use_despiked and the same chain called by hand, bit for bit;
    and T differs from the chain's without the switch."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "1"])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    runs = []
    for despike in (True, False):
        r = pkg.Renderer()
        r.upload(s) if despike else r.share_scene(runs[0][0])
        if despike:
            r.track_motion(True)
        r.resize(w, h)
        runs.append((r, []))
    owner, base = runs[0][0], runs[1][0]
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        owner.update_animation(it, bn if len(bn) else None)
        for r, out in runs:
            r.reset()
            for f in range(spp):
                r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
            if r is owner:
                r.despike()  # DESPIKE_DEFAULTS are the adapter's (the header test holds them together)
                r.chain_use_despiked(True)
            r.render_guides_motion(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=spp))
            view, proj = s.camera_matrices(w, h)
            r.temporal_accumulate_motion(spp, view, proj, max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
            r.denoise_temporal(iterations=3, sigma_color=1.5, sigma_normal=0.3, sigma_position=0.03)
            r.postprocess_denoised(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
            out.append((r.readback(), r.read_temporal(), r.read_output(pkg.OUTPUT_RGBA32F)))
        differ = [int((_bits(a) != _bits(b)).any(axis=-1).sum()) for a, b in zip(got[frame], runs[0][1][frame])]
        print(f"frame {frame}: pixels differing in the sum, T and the output image {differ}")
        assert differ == [0, 0, 0], frame
        assert (_bits(runs[0][1][frame][0]) == _bits(runs[1][1][frame][0])).all()  # the sum is nobody's to change
    changed = (_bits(runs[0][1][1][1]) != _bits(runs[1][1][1][1])).any(axis=-1)
    print(f"second frame: T differs from the chain's without the switch on {int(changed.sum())} pixels")
    assert changed.sum() > 20
    base.close()
    owner.close()


@pytest.mark.gpu
def test_renderer_hip_without_a_denoiser_despikes_ahead_of_the_output_stage(pkg, tmp_path_factory, tmp_path):
    """The same driver with FireflySettings on and every other setting off: the output image of both frames equals ptx_despike at the
    adapter's defaults followed by ptx_postprocess_despiked, bit for bit, and differs from ptx_postprocess' on the sum."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "1", "0"])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(w, h)
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        r.update_animation(it, bn if len(bn) else None)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
        r.despike()
        r.postprocess_despiked(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        S, out = r.readback(), r.read_output(pkg.OUTPUT_RGBA32F)
        assert (_bits(got[frame][0]) == _bits(S)).all() and (_bits(got[frame][2]) == _bits(out)).all(), frame
        r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) != _bits(out)).any()
    r.close()
