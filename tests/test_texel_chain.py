"""Texel production (k_build_srgb_lut, k_blit_level, k_decode_texels, k_stream_chain, k_alpha_quads, k_alpha_tris) and the
any-hit alpha lookup (hitAlpha) against tests/texel_ref.py: a float64 restatement of the Vulkan definitions that shares
nothing with the kernels or with the oracle.  The oracle is held to the same reference by the CPU tests.

THE COMPARISON RULES (used by every test below)

Reading a level back.  Level k of a texture is read through test_texture at texel centres with dudx = 2^k / w, dvdy = 2^k / h.
The float32 inputs are chosen so that u * w is exactly i + 1/2 and dudx * w exactly 2^k wherever such a float32 exists (it
does for every float case here: the lookup then returns the texel itself).  An 8-bit level becomes bytes by the nearest
decodable value, which must lie within 1e-5 (the smallest gap between two decodable values is 3.0e-4, sRGB codes 0 and 1).
Float levels are compared as values.

Per-level step.  Level 0 equals the caller's bytes.  The reference for level l is the blit of the bytes read back at level
l - 1, so one tie flip does not compound down the chain.

Tie rule.  With v the float64 value about to be stored, in code units: a texel-channel is excused iff
|(v + 1/2) - round(v + 1/2)| <= m, m = 8 * M_TIE; an excused one must be floor(v) or floor(v) + 1, every other one
floor(v + 1/2).  M_TIE is the largest |v32 - v64| of the reference alone over the case list (float32 against float64 from the
same bytes), recorded below and recomputed by a CPU test.

Float textures.  |got - v| <= max(8 * M_F32, 2^-20) * max(1, |v|), M_F32 measured the same way.

Caps on the excused share, per channel class, asserted for every level of at least 256 texel-channels (smaller levels get the
rule without a cap): sRGB colour channels <= 1 %, linear channels (UNORM, sRGB alpha) <= 30 % (a 2 x 2 mean of bytes ties
exactly when the four sum to 2 mod 4: 25 %).  The two tie-free images have no such block, and their level 1 is held to
<= 1 % in every class.  The excused and non-excused counts of every level are printed (pytest -s), so a run that excused
nearly everything is visible.  A capped level can be as small as 8 x 8, where the alpha class of an sRGB image has 64
channels and 25 % of ties is 16 +- 3.5 against a cap of 19: the seeds of the images are chosen so that the reference's own
chains stay clear of the caps (EXCUSED_SHARES, held by test_recorded_excused_shares).

The inputs.  M_TIE is set by the worst step of the list, and that is a scaled blit: a float32 texel coordinate near 37 carries
2e-6 of rounding, which neighbours 255 codes apart turn into 5e-4 of a code.  With independent random bytes at the odd extents
the margin 8 * 5.2e-4 excused 0.8 % - 1.6 % of the sRGB colour channels by the reference alone, more than the cap allows; as
the cap is the condition and the input the variable, the images with an odd extent in their chain are random fields over the
whole byte range plus independent noise of +-40 (_random_bytes).  The 64 x 64, tie-free and tiny images are independent bytes.

Scaled-down uploads.  Only level 0 of the result is observable, so the reference chains its own quantised steps.  Every step
is monotone in every source texel-channel (weights >= 0, monotone transfer functions): the chain that stores
floor(v + 1/2 - m) at every step bounds the result from below, the chain that stores floor(v + 1/2 + m) from above, and the
stored code must lie between the two.  Where they agree the code is decided; where they differ (by one code) the texel-channel
is excused.  This excuses a result whose last step had an excused source only if that source can change the code, and follows a
tie through more than one step, which "excused when a source of the last step was excused" does not.  <= 1 %.

Any-hit.  With a the float64 alpha: a closest ray is excused iff 0 < |a - 0.5| <= m_a, a shadow ray iff 0 < |a - 1| <= m_a,
m_a = 8 * M_ALPHA (the reference alone, float32 barycentrics and float32 arithmetic against float64); a == 1 exactly (a
footprint of four 255s under a factor of 1) is never excused.  A ray that passes within 1e-4 (barycentric) of a quad's
outline is excused as well.  An excused closest ray may report only what a reading of the quads in the band or grazed allows:
the nearest kept quad with those quads kept, the same with them left out, or a grazed quad.  At most 2 % of a case's rays
may be excused (EXCUSED_RAYS records the shares)."""
import ctypes as C

import numpy as np
import pytest

import texel_ref as ref
import util
from test_textures import _desc_with, _inputs
from texel_ref import F32, SRGB, UNORM

# ---------------------------------------------------------------------------------------
# recorded constants (measured on the CPU from the reference alone; test_recorded_constants recomputes them)
# ---------------------------------------------------------------------------------------
M_TIE = 1.8e-4      # code units
M_F32 = 1.3e-7      # relative to max(1, |v|)
M_ALPHA = 2.2e-5
SRGB_TABLE_ERR = 1.9e-7   # the oracle's decoded 256 x 1 sRGB ramp against the closed form (test_srgb_table_...)
UNLIMITED = 2**64 - 1
# the largest share of excused rays over the slots of the any-hit scene, by the reference alone (cap 2 %)
EXCUSED_RAYS = {"closest": 0.0008, "shadow": 0.0016}


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
def _tie_free(img):
    """Nudge one byte of every 2 x 2 block whose four bytes sum to 2 mod 4, per channel."""
    img = img.astype(np.int64)
    s = img[0::2, 0::2] + img[1::2, 0::2] + img[0::2, 1::2] + img[1::2, 1::2]
    tie = s % 4 == 2
    c = img[0::2, 0::2]
    c[tie] += np.where(c[tie] < 255, 1, -1)
    return img.astype(np.uint8)


def _random_bytes(rng, w, h):
    """Random bytes.  Where every step of the chain halves an even extent (or the image is tiny) they are independent; where
    a step is a scaled blit they are a random field over the whole byte range plus independent noise of +-40, which limits the
    difference between neighbours: a float32 texel coordinate near 64 carries 4e-6 of rounding, which random neighbours (a
    difference of up to 255 codes) turn into 1e-3 of a code, and the tie margin -- set by the worst case of the list -- then
    excuses more than the caps allow by the reference alone."""
    if max(w, h) <= 8 or all(e % 2 == 0 or e == 1 for d in ref.chain_dims(w, h) for e in d):
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    gw, gh = w // 6 + 2, h // 6 + 2
    coarse = rng.uniform(-30, 285, (gh, gw, 4))
    x, y = np.arange(w) / 6.0, np.arange(h) / 6.0
    i, j, ax, ay = x.astype(int), y.astype(int), (x % 1)[None, :, None], (y % 1)[:, None, None]
    field = (coarse[j][:, i] * (1 - ax) + coarse[j][:, i + 1] * ax) * (1 - ay) + (coarse[j + 1][:, i] * (1 - ax) + coarse[j + 1][:, i + 1] * ax) * ay
    return np.clip(np.round(field + rng.integers(-40, 41, (h, w, 4))), 0, 255).astype(np.uint8)


def _chain_cases(seed=2034):
    """(id, w, h, format, texels (h, w, 4))"""
    rng = np.random.default_rng(seed)
    # the seeds: the capped levels go down to 8 x 8 (64 alpha channels of an sRGB image, 25 % of ties is 16 +- 3.5, the cap 19);
    # these keep the shares of the reference's own chains (EXCUSED_SHARES) clear of the caps
    rng64 = np.random.default_rng(3013)
    square = {fmt: rng64.integers(0, 256, (64, 64, 4)).astype(np.uint8) for fmt in (SRGB, UNORM)}
    out = []
    for w, h in ((64, 64), (37, 21), (33, 7), (5, 3), (100, 1), (1, 100), (130, 66), (2, 2), (1, 1)):
        for fmt in (SRGB, UNORM):
            out.append((f"{w}x{h}-{'srgb' if fmt == SRGB else 'unorm'}", w, h, fmt, square[fmt] if w == 64 else _random_bytes(rng, w, h)))
    for fmt in (SRGB, UNORM):
        out.append((f"64x64-{'srgb' if fmt == SRGB else 'unorm'}-tiefree", 64, 64, fmt, _tie_free(rng64.integers(0, 256, (64, 64, 4)))))
    for w, h in ((34, 18), (32, 32)):
        out.append((f"{w}x{h}-f32", w, h, F32, rng.uniform(0, 4, (h, w, 4)).astype(np.float32)))
    return out


def _scaled_cases():
    """(id, w, h, format, texels, per-texture share, planned extent, halvings, final blit)"""
    rng = np.random.default_rng(2034)

    def srgb(w, h):
        px = _random_bytes(rng, w, h)
        px[..., 3] = 255
        return px

    return [
        ("37x21-srgb-share2000", 37, 21, SRGB, srgb(37, 21), 2000, (12, 7), 1, True),
        ("37x21-srgb-share6000", 37, 21, SRGB, srgb(37, 21), 6000, (18, 10), 1, False),
        ("100x60-srgb-share6000", 100, 60, SRGB, srgb(100, 60), 6000, (25, 15), 2, False),
        ("100x60-srgb-share1200", 100, 60, SRGB, srgb(100, 60), 1200, (7, 4), 3, True),
        ("64x16-f32-share6000", 64, 16, F32, rng.uniform(0, 4, (16, 64, 4)).astype(np.float32), 6000, (16, 4), 2, False),
    ]


CHAIN_CASES = _chain_cases()
SCALED_CASES = _scaled_cases()
STREAMED = ("64x64-srgb", "64x64-unorm", "130x66-srgb", "130x66-unorm", "37x21-srgb", "37x21-unorm", "100x1-srgb", "100x1-unorm", "34x18-f32")

# the largest excused share per case (sRGB colour, linear) over the levels the caps apply to, of the reference's own chain:
# recorded, recomputed by test_recorded_excused_shares (see docs/NEXT_ROWS.md section 7 for the table)
EXCUSED_SHARES = {
    "64x64-srgb": (0.0026, 0.2695), "64x64-unorm": (0.0, 0.2646), "37x21-srgb": (0.0037, 0.0111), "37x21-unorm": (0.0, 0.0028),
    "33x7-srgb": (0.0, 0.0), "33x7-unorm": (0.0, 0.0), "5x3-srgb": (0.0, 0.0), "5x3-unorm": (0.0, 0.0),
    "100x1-srgb": (0.0, 0.0), "100x1-unorm": (0.0, 0.0), "1x100-srgb": (0.0, 0.0), "1x100-unorm": (0.0, 0.0),
    "130x66-srgb": (0.0059, 0.2522), "130x66-unorm": (0.0, 0.2526), "2x2-srgb": (0.0, 0.0), "2x2-unorm": (0.0, 0.0),
    "1x1-srgb": (0.0, 0.0), "1x1-unorm": (0.0, 0.0), "64x64-srgb-tiefree": (0.0065, 0.2344), "64x64-unorm-tiefree": (0.0, 0.2568),
    # scaled-down uploads whose result has at least 256 texel-channels (100 x 60 -> 7 x 4 has 112: the rule without a cap)
    "37x21-srgb-share2000": (0.004, 0.0), "37x21-srgb-share6000": (0.0, 0.0), "100x60-srgb-share6000": (0.0027, 0.0),
}


# ---------------------------------------------------------------------------------------
# reading a level back
# ---------------------------------------------------------------------------------------
def _exact_factor(target, n):
    """float32 g next to target / n with float32(g * float32(n)) == target, where one exists (else the nearest)."""
    f = np.float32
    target = np.asarray(target, np.float64)
    g0 = (target / n).astype(np.float32)
    best, found = g0.copy(), np.zeros(g0.shape, bool)
    for cand in (g0, np.nextafter(g0, f(np.inf)), np.nextafter(g0, f(-np.inf)), np.nextafter(np.nextafter(g0, f(np.inf)), f(np.inf)),
                 np.nextafter(np.nextafter(g0, f(-np.inf)), f(-np.inf))):
        ok = ((cand * f(n)).astype(np.float32) == target) & ~found
        best = np.where(ok, cand, best)
        found |= ok
    return best, found


def _read_level(sample, w, h, k, need_exact=False):
    """Level k of the one texture (shader index 9) of extent w x h as the sampler sees it: float32 (h_k, w_k, 4)."""
    lw, lh = max(w >> k, 1), max(h >> k, 1)
    ys, xs = np.mgrid[0:lh, 0:lw]
    u, fu = _exact_factor(xs.reshape(-1) + 0.5, lw)
    v, fv = _exact_factor(ys.reshape(-1) + 0.5, lh)
    gx, fx = _exact_factor(np.float64(2.0 ** k), w)
    gy, fy = _exact_factor(np.float64(2.0 ** k), h)
    assert fx and fy, "no float32 gradient puts the lookup on the level exactly"
    if need_exact:
        assert fu.all() and fv.all()
    if w == 1 and h == 1:
        out = sample(_inputs(9, u, v), True)
    else:
        out = sample(_inputs(9, u, v, dudx=gx, dvdy=gy), False)
    return out.view(np.float32).reshape(lh, lw, 4)


_DECODABLE = {UNORM: np.arange(256) / 255.0, SRGB: ref.srgb_to_linear(np.arange(256) / 255.0)}


def _to_bytes(level, fmt):
    """The bytes behind a level read back as decoded float32 values."""
    out = np.zeros(level.shape, np.int64)
    worst = 0.0
    for c in range(4):
        table = _DECODABLE[SRGB if fmt == SRGB and c < 3 else UNORM]
        x = level[..., c].astype(np.float64)
        i = np.clip(np.searchsorted(table, x), 1, 255)
        i = np.where(np.abs(table[i - 1] - x) <= np.abs(table[i] - x), i - 1, i)
        worst = max(worst, float(np.abs(table[i] - x).max()))
        out[..., c] = i
    assert worst < 1e-5, f"a texel read back lies {worst} from the nearest decodable value"
    return out


def _classes(fmt, shape):
    """Boolean masks (srgb colour, linear) over an (h, w, 4) level."""
    colour = np.zeros(shape, bool)
    if fmt == SRGB:
        colour[..., :3] = True
    return colour, ~colour


def _tie_rule(v, got, fmt, label, cap_linear=0.30, cap_colour=0.01, always_cap=False):
    """Hold the codes `got` to the float64 pre-quantisation values `v`; returns {class: (excused, non-excused)}."""
    m = 8 * M_TIE
    excused = np.abs((v + 0.5) - np.round(v + 0.5)) <= m
    lo = np.floor(v).astype(np.int64)
    want = np.floor(v + 0.5).astype(np.int64)
    ok = np.where(excused, (got == lo) | (got == lo + 1), got == want)
    assert ok.all(), f"{label}: {int((~ok).sum())} of {ok.size} texel-channels break the tie rule, first {np.argwhere(~ok)[0]}: " \
                     f"v = {v[tuple(np.argwhere(~ok)[0])]!r}, stored {got[tuple(np.argwhere(~ok)[0])]}"
    return _count_and_cap(excused, fmt, label, cap_linear, cap_colour, always_cap)


def _count_and_cap(excused, fmt, label, cap_linear=0.30, cap_colour=0.01, always_cap=False):
    """{class: (excused, non-excused)} of one level, printed (pytest -s shows a run that excused nearly everything), with the
    caps asserted where the level has at least 256 texel-channels."""
    counts = {}
    for name, mask, cap in zip(("colour", "linear"), _classes(fmt, excused.shape), (cap_colour, cap_linear)):
        n = int(mask.sum())
        e = int((excused & mask).sum())
        counts[name] = (e, n - e)
        if n and (excused.size >= 256 or always_cap):
            assert e <= cap * n, f"{label}: {e} of {n} {name} texel-channels excused (cap {cap})"
    capped = excused.size >= 256 or always_cap
    print(f"{label}: sRGB colour {counts['colour'][0]} excused, {counts['colour'][1]} not; linear {counts['linear'][0]} excused, "
          f"{counts['linear'][1]} not{'' if capped else ' (fewer than 256 texel-channels: no cap)'}")
    return counts


def _float_rule(v, got, label):
    tol = max(8 * M_F32, 2.0 ** -20) * np.maximum(1.0, np.abs(v))
    err = np.abs(np.float64(got) - v)
    assert (err <= tol).all(), f"{label}: {int((err > tol).sum())} texels off, worst {float((err / tol).max())} tolerances"


def _check_chain(sample, case):
    name, w, h, fmt, texels = case
    dims = ref.chain_dims(w, h)
    assert dims[-1] == (1, 1) and dims[0] == (w, h)
    counts = []
    if fmt == F32:
        above = _read_level(sample, w, h, 0, need_exact=True)
        assert (above == texels).all(), f"{name}: level 0 is not the caller's texels"
        for l in range(1, len(dims)):
            v, _ = ref.blit_step(above, fmt, *dims[l])
            got = _read_level(sample, w, h, l, need_exact=True)
            _float_rule(v, got, f"{name} level {l}")
            above = got
        return counts
    above = _to_bytes(_read_level(sample, w, h, 0), fmt)
    assert (above == texels).all(), f"{name}: level 0 is not the caller's bytes"
    for l in range(1, len(dims)):
        v, _ = ref.blit_step(above, fmt, *dims[l])
        got = _to_bytes(_read_level(sample, w, h, l), fmt)
        tie_free = "tiefree" in name and l == 1
        counts.append(_tie_rule(v, got, fmt, f"{name} level {l}", cap_linear=0.01 if tie_free else 0.30, always_cap=tie_free))
        above = got
    return counts


def _reference_scaled(case):
    """The scaled-down path on the reference's own quantised steps: (v of the last step, lowest code, highest code).  Every
    step is monotone in every source texel-channel (weights >= 0, monotone transfer functions), so the chain that stores
    floor(v + 1/2 - m) at every step bounds what an implementation within the tie rule can hold from below, and the chain that
    stores floor(v + 1/2 + m) from above.  Where the two agree the code is decided; elsewhere the texel-channel is excused."""
    name, w, h, fmt, texels, share, extent, halvings, final_blit = case
    plan = ref.planned_extent(w, h, fmt, share)
    assert (plan["extent"], plan["halvings"], plan["final_blit"]) == (extent, halvings, final_blit)
    m = 8 * M_TIE
    nom = lo = hi = texels
    v = None
    for dw, dh in ref.scaled_steps(w, h, plan):
        v, code = ref.blit_step(nom, fmt, dw, dh)
        if fmt == F32:
            nom = lo = hi = v.astype(np.float32)   # a float level is stored as binary32
        else:
            lo = np.clip(np.floor(ref.blit_step(lo, fmt, dw, dh)[0] + 0.5 - m), 0, 255).astype(np.int64)
            hi = np.clip(np.floor(ref.blit_step(hi, fmt, dw, dh)[0] + 0.5 + m), 0, 255).astype(np.int64)
            nom = code
    return v, lo, hi


def _check_scaled(sample, case):
    name, w, h, fmt, texels, share, extent, halvings, final_blit = case
    ew, eh = extent
    v, lo, hi = _reference_scaled(case)
    if fmt == F32:
        _float_rule(v, _read_level(sample, ew, eh, 0, need_exact=True), name)
        return None
    got = _to_bytes(_read_level(sample, ew, eh, 0), fmt)
    ok = (got >= lo) & (got <= hi)
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.size} texel-channels outside what the tie rule allows, first {np.argwhere(~ok)[0]}"
    assert (hi - lo <= 1).all()
    return _count_and_cap(lo != hi, fmt, name, cap_linear=0.01)


def _one_texture_desc(pkg, scene, w, h, fmt, texels, budget=UNLIMITED, levels=1, force_full=False):
    flat = np.ascontiguousarray(texels).reshape(-1)
    return _desc_with(pkg, scene, [(w, h, fmt, levels, flat)], budget=budget, force_full=force_full)


@pytest.fixture(scope="module")
def base_scene(pkg):
    return pkg.Scene("texture_test")


# ---------------------------------------------------------------------------------------
# CPU: the reference alone
# ---------------------------------------------------------------------------------------
def test_planned_extent_known_answers():
    assert ref.chain_bytes(32, SRGB) == 5460 and ref.chain_bytes(64, UNORM) == 21844 and ref.chain_bytes(16, F32) == 5456
    assert [ref.max_extent(SRGB, s) for s in (6000, 2000, 1200, 5460, 5459, 1364, 1363, 3, UNLIMITED)] == [32, 16, 8, 32, 16, 16, 8, 1, 4096]
    assert ref.max_extent(F32, 6000) == 16 and ref.max_extent(F32, 1200) == 4 and ref.max_extent(F32, 6000, force_full=True) == 4096
    for name, w, h, fmt, _, share, extent, halvings, final_blit in SCALED_CASES:
        p = ref.planned_extent(w, h, fmt, share)
        assert (p["extent"], p["halvings"], p["final_blit"], p["skipped"]) == (extent, halvings, final_blit, None), name
    assert ref.scaled_steps(37, 21, ref.planned_extent(37, 21, SRGB, 2000)) == [(18, 10), (12, 7)]
    assert ref.scaled_steps(100, 60, ref.planned_extent(100, 60, SRGB, 1200)) == [(50, 30), (25, 15), (12, 7), (7, 4)]
    # a file's complete chain gives up its first levels; an incomplete one is not used; a texture that fits is untouched
    p = ref.planned_extent(64, 64, SRGB, 6000, file_levels=7)
    assert (p["extent"], p["scale"], p["skipped"], p["halvings"]) == ((32, 32), 2, 1, 0)
    assert ref.planned_extent(64, 64, SRGB, 6000, file_levels=3)["skipped"] is None
    assert ref.planned_extent(8, 8, UNORM, 6000, file_levels=4) == dict(extent=(8, 8), scale=1, halvings=0, final_blit=False, skipped=0)
    assert ref.planned_extent(8, 8, UNORM, 6000, file_levels=2)["skipped"] is None
    assert ref.planned_extent(64, 64, SRGB, 6000, force_full=True)["extent"] == (64, 64)
    assert ref.planned_extent(600, 4, SRGB, 1_400_000)["extent"] == (300, 2) and ref.planned_extent(300, 2, SRGB, 1_400_000)["scale"] == 1
    assert ref.planned_extent(5000, 3, UNORM, UNLIMITED)["extent"] == (2500, 1)
    assert ref.chain_dims(37, 21) == [(37, 21), (18, 10), (9, 5), (4, 2), (2, 1), (1, 1)]
    assert ref.chain_dims(100, 1) == [(100, 1), (50, 1), (25, 1), (12, 1), (6, 1), (3, 1), (1, 1)] and ref.chain_dims(1, 1) == [(1, 1)]


def test_reference_blit_known_answers():
    """The reference against hand-worked numbers: an even halving is the 2 x 2 mean; 3 -> 1 reads the middle texel; 5 -> 2 has
    weights 1/4, 3/4 at the first texel; 1 -> 3 replicates the texel (clamp at both edges); sRGB round-trips every code."""
    rng = np.random.default_rng(1)
    a = rng.uniform(0, 1, (6, 8, 4))
    assert np.allclose(ref.blit(a, 4, 3), (a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2]) / 4, atol=1e-15)
    row = np.zeros((1, 3, 4))
    row[0, :, 0] = [1, 10, 100]
    assert ref.blit(row, 1, 1)[0, 0, 0] == 10
    row5 = np.zeros((1, 5, 4))
    row5[0, :, 0] = [1, 2, 4, 8, 16]
    assert np.allclose(ref.blit(row5, 2, 1)[0, :, 0], [0.25 * 1 + 0.75 * 2, 0.75 * 8 + 0.25 * 16], atol=1e-15)
    assert (ref.blit(row[:, :1], 3, 1)[0, :, 0] == 1).all()
    edge = ref.blit(row5, 9, 1)[0, :, 0]
    assert edge[0] == 1 and edge[-1] == 16
    codes = np.arange(256)
    assert (ref.quantise(ref.linear_to_srgb(ref.srgb_to_linear(codes / 255.0)) * 255) == codes).all()
    assert abs(ref.srgb_to_linear(np.float64(0.04045)) - 0.04045 / 12.92) < 1e-15 and abs(ref.srgb_to_linear(np.float64(1.0)) - 1.0) < 1e-15
    assert abs(ref.linear_to_srgb(np.float64(0.0031308)) - 0.0031308 * 12.92) < 1e-15
    assert ref.blit(a.astype(np.float32), 3, 2).dtype == np.float32 and ref.srgb_to_linear(np.float32([0.5])).dtype == np.float32
    # the tie-free images have no 2 x 2 block summing to 2 mod 4
    for c in CHAIN_CASES:
        if "tiefree" in c[0]:
            t = c[4].astype(np.int64)
            assert ((t[0::2, 0::2] + t[1::2, 0::2] + t[0::2, 1::2] + t[1::2, 1::2]) % 4 != 2).all()


def test_one_minus_t_plus_t_is_one_in_binary32():
    """(1 - t) + t == 1 in binary32 for every t in [0, 1]: four texels of 255 interpolate to exactly 1 whatever the weights.
    All 2^23 fractions of [0.5, 1), every 2^-24 step of [0, 0.5) taken 2^23 at a stride, and 2^22 random bit patterns below 1."""
    f = np.float32
    t = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F000000)).view(np.float32)
    assert (((f(1) - t) + t) == f(1)).all()
    t = np.arange(1 << 23, dtype=np.float32) * f(2.0 ** -24)
    assert (((f(1) - t) + t) == f(1)).all()
    rng = np.random.default_rng(3)
    t = rng.integers(0, 0x3F800001, 1 << 22, dtype=np.uint32).view(np.float32)
    assert (((f(1) - t) + t) == f(1)).all()
    # and the bilinear of four ones is one, in both precisions
    one = np.ones((2, 2))
    for dt in (np.float32, np.float64):
        a, all_one = ref.alpha_at(one.astype(dt), 2, 2, rng.uniform(-3, 3, 1000).astype(dt), rng.uniform(-3, 3, 1000).astype(dt), 1.0)
        assert (a == 1).all() and all_one.all()


def _measure_m_tie_and_f32():
    """The reference in float32 against itself in float64, step by step from the same stored texels, over every case."""
    runs = [(texels, fmt, ref.chain_dims(w, h)[1:]) for name, w, h, fmt, texels in CHAIN_CASES]
    runs += [(texels, fmt, ref.scaled_steps(w, h, ref.planned_extent(w, h, fmt, share))) for name, w, h, fmt, texels, share, *_ in SCALED_CASES]
    m_tie = m_f32 = 0.0
    for cur, fmt, steps in runs:
        for dw, dh in steps:
            v64, code = ref.blit_step(cur, fmt, dw, dh, np.float64)
            v32, _ = ref.blit_step(cur, fmt, dw, dh, np.float32)
            if fmt == F32:
                m_f32 = max(m_f32, float((np.abs(v32 - v64) / np.maximum(1, np.abs(v64))).max()))
                cur = v64.astype(np.float32)
            else:
                m_tie = max(m_tie, float(np.abs(v32 - v64).max()))
                cur = code
    return m_tie, m_f32


def _reference_excused_shares():
    """Per case the largest excused share (colour, linear) over the capped levels of the reference's own chain."""
    out = {}
    for name, w, h, fmt, texels in CHAIN_CASES:
        if fmt == F32:
            continue
        cur, worst = texels, [0.0, 0.0]
        for dw, dh in ref.chain_dims(w, h)[1:]:
            v, code = ref.blit_step(cur, fmt, dw, dh)
            excused = np.abs((v + 0.5) - np.round(v + 0.5)) <= 8 * M_TIE
            for k, mask in enumerate(_classes(fmt, v.shape)):
                if v.size >= 256 and mask.any() and not ("tiefree" in name and dw == 32):
                    worst[k] = max(worst[k], float((excused & mask).sum() / mask.sum()))
            cur = code
        out[name] = (round(worst[0], 4), round(worst[1], 4))
    for case in SCALED_CASES:
        if case[3] != F32:
            v, lo, hi = _reference_scaled(case)
            if v.size >= 256:
                out[case[0]] = (round(float((lo != hi)[..., :3].mean()), 4), round(float((lo != hi)[..., 3].mean()), 4))
    return out


def test_recorded_constants():
    m_tie, m_f32 = _measure_m_tie_and_f32()
    m_alpha = _alpha_scene_reference()["m_alpha"]
    print(f"M_TIE {m_tie:.3e} M_F32 {m_f32:.3e} M_ALPHA {m_alpha:.3e}")
    for name, got, recorded in (("M_TIE", m_tie, M_TIE), ("M_F32", m_f32, M_F32), ("M_ALPHA", m_alpha, M_ALPHA)):
        assert recorded / 2 <= got <= recorded * 2, (name, got, recorded)


def test_recorded_excused_shares():
    got = _reference_excused_shares()
    print(got)
    assert got.keys() == EXCUSED_SHARES.keys()
    for name, (colour, linear) in got.items():
        # the caps themselves, and the recorded figures within what one texel-channel of the smallest capped class moves
        assert colour <= 0.01 and linear <= (0.01 if "share" in name else 0.30), name
        assert abs(colour - EXCUSED_SHARES[name][0]) <= 0.006 and abs(linear - EXCUSED_SHARES[name][1]) <= 0.02, name


# ---------------------------------------------------------------------------------------
# CPU: the oracle against the reference
# ---------------------------------------------------------------------------------------
def _oracle_sampler(orc, desc):
    osc = orc.OracleScene(desc, build_bvh=False)
    return lambda inp, implicit: osc.test_texture(inp, implicit)


@pytest.mark.parametrize("k", range(len(CHAIN_CASES)), ids=[c[0] for c in CHAIN_CASES])
def test_oracle_chain_against_float64_blit(pkg, orc, base_scene, k):
    case = CHAIN_CASES[k]
    d, keep = _one_texture_desc(pkg, base_scene, *case[1:5])
    _check_chain(_oracle_sampler(orc, d), case)


@pytest.mark.parametrize("k", range(len(SCALED_CASES)), ids=[c[0] for c in SCALED_CASES])
def test_oracle_scaled_upload_against_float64_blit(pkg, orc, base_scene, k):
    case = SCALED_CASES[k]
    d, keep = _one_texture_desc(pkg, base_scene, *case[1:5], budget=case[5])
    _check_scaled(_oracle_sampler(orc, d), case)


def _file_chain_case():
    rng = np.random.default_rng(2026)
    levels = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for w, h in ref.chain_dims(64, 64)]
    return levels, np.concatenate([l.reshape(-1) for l in levels])


def _check_file_chain_and_force_full(pkg, base_scene, sampler_of):
    levels, data = _file_chain_case()
    p = ref.planned_extent(64, 64, SRGB, 6000, file_levels=7)
    assert p["extent"] == (32, 32) and p["skipped"] == 1
    d, keep = _one_texture_desc(pkg, base_scene, 64, 64, SRGB, data, budget=6000, levels=7)
    sample = sampler_of(d)
    for k in range(6):  # level k of the image = level k + skipped of the file, byte for byte
        assert (_to_bytes(_read_level(sample, 32, 32, k), SRGB) == levels[k + 1]).all(), k
    d, keep = _one_texture_desc(pkg, base_scene, 64, 64, SRGB, data, budget=6000, levels=7, force_full=True)
    sample = sampler_of(d)
    for k in range(7):
        assert (_to_bytes(_read_level(sample, 64, 64, k), SRGB) == levels[k]).all(), k
    # forceFullTextureSize on an image without a chain: the unscaled bytes and their generated chain
    case = next(c for c in CHAIN_CASES if c[0] == "37x21-srgb")
    d, keep = _one_texture_desc(pkg, base_scene, *case[1:5], budget=1200, force_full=True)
    _check_chain(sampler_of(d), case)


def test_oracle_file_chain_under_a_budget_and_force_full(pkg, orc, base_scene):
    _check_file_chain_and_force_full(pkg, base_scene, lambda d: _oracle_sampler(orc, d))


def test_srgb_table_against_the_closed_form(pkg, orc, base_scene):
    """test_texture on a 256 x 1 sRGB ramp: what k_build_srgb_lut's twin in the oracle decodes, against the closed form in
    float64.  Measured maximum 1.87e-7 (SRGB_TABLE_ERR), at code 246; held to 8 x that."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 4, axis=2)
    d, keep = _one_texture_desc(pkg, base_scene, 256, 1, SRGB, ramp)
    got = _read_level(_oracle_sampler(orc, d), 256, 1, 0, need_exact=True)[0]
    want = ref.srgb_to_linear(np.arange(256) / 255.0)
    err = float(np.abs(got[:, :3] - want[:, None]).max())
    print(f"sRGB table error {err:.3e}")
    assert err <= 8 * SRGB_TABLE_ERR
    assert np.abs(got[:, 3] - np.arange(256) / 255.0).max() <= 2.0 ** -24  # alpha is b / 255, correctly rounded
    assert got[0, 0] == 0 and got[255, 0] == 1


# ---------------------------------------------------------------------------------------
# the any-hit scene
# ---------------------------------------------------------------------------------------
_ALPHAS = np.uint8([0, 90, 127, 128, 200, 254, 255])
WALL_Z, RAY_Z = 1.0, -5.0


def _alpha_texture(rng, w, h, islands=(), p=None):
    px = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    px[..., 3] = rng.choice(_ALPHAS, (h, w), p=p)
    for x0, x1, y0, y1 in islands:
        px[y0:y1, x0:x1, 3] = 255
    return px


def _alpha_textures():
    rng = np.random.default_rng(77)
    t = [
        _alpha_texture(rng, 37, 21, [(3, 18, 4, 13), (24, 34, 12, 20)]),
        _alpha_texture(rng, 300, 2, [(40, 140, 0, 2), (200, 230, 0, 2)]),
        _alpha_texture(rng, 64, 64, [(10, 40, 10, 40)]),
        _alpha_texture(rng, 2, 1),
        _alpha_texture(rng, 1, 1),
        _alpha_texture(rng, 37, 21, [(5, 14, 2, 9)], p=(0.3, 0.3, 0.1, 0.1, 0.1, 0.05, 0.05)),   # mostly holes: the quad behind shows
        _alpha_texture(rng, 600, 4, [(100, 300, 0, 4), (420, 500, 0, 4)]),   # 300 x 2 under the budget below
        _alpha_texture(rng, 2, 2),
    ]
    t[3][0, :, 3] = (255, 0)
    t[4][0, 0, 3] = 255
    t[7][..., 3] = 255
    return t


# the per-texture share that makes 512 the largest RGBA8 extent: only the 600 x 4 texture is scaled
ALPHA_SHARE = 1_400_000
MR, SG, PHONG = 0, 1, 2
# (name, texture, slot along x, z, (u range, v range), mirrored and swapped, material type, colour factor alpha)
QUADS = [
    ("37x21", 0, 0, -0.10, (-1.5, 2.5), False, MR, 1.0),
    ("300x2", 1, 1, -0.15, (0.0, 1.0), False, SG, 1.0),
    ("64x64 x 0.9", 2, 2, -0.20, (-0.5, 1.5), False, PHONG, 0.9),
    ("2x1", 3, 3, -0.25, (-3.0, 3.0), False, MR, 1.0),
    ("1x1 x 0.6", 4, 4, -0.30, (0.0, 1.0), False, SG, 0.6),
    ("37x21 mirrored, in front", 5, 5, -0.60, (-1.5, 2.5), True, PHONG, 1.0),
    ("600x4 scaled, behind", 6, 5, -0.35, (0.0, 1.0), False, MR, 1.0),
    ("2x2 of 255 x 0.5", 7, 6, -0.40, (0.0, 1.0), False, SG, 0.5),
]
SLOTS = 7


def _quad_corners(slot, z):
    x0 = 3.0 * slot
    return np.float32([[x0, 0, z], [x0 + 2, 0, z], [x0 + 2, 2, z], [x0, 2, z]])


def _quad_uv(rng_uv, mirrored):
    lo, hi = rng_uv
    cx, cy = np.float32([0, 1, 1, 0]), np.float32([0, 0, 1, 1])
    if mirrored:  # u runs down the quad's y, v along its x
        return np.stack([hi - (hi - lo) * cy, lo + (hi - lo) * cx], 1).astype(np.float32)
    return np.stack([lo + (hi - lo) * cx, lo + (hi - lo) * cy], 1).astype(np.float32)


class AlphaScene:
    """An opaque wall at z = 1 and the non-opaque quads of QUADS in front of it: a PtxSceneDesc whose arrays this object keeps."""

    def __init__(self, pkg, pending=False):
        wall = util.quad_mesh(np.float32([[-10, -10, WALL_Z], [40, -10, WALL_Z], [40, 12, WALL_Z], [-10, 12, WALL_Z]]), (0, 0, 1))
        meshes = [wall]
        for name, tex, slot, z, uvr, mirrored, mtype, factor in QUADS:
            q = util.quad_mesh(_quad_corners(slot, z), (0, 0, 1))
            q["uv"] = _quad_uv(uvr, mirrored)
            meshes.append(q)
        self.soup = util.TriangleSoup(pkg, [meshes])
        self.soup.geometries["IsOpaque"][1:] = 0
        mats = {MR: [util.mr_material()], SG: [], PHONG: []}
        ids = [0]
        for name, tex, slot, z, uvr, mirrored, mtype, factor in QUADS:
            m = util.mr_material(color=(0.8, 0.7, 0.6))
            m[7] = factor
            if mtype != MR:  # specular-glossiness / Phong: the texture slots sit one word earlier
                m[8:18] = (0.5, 0.5, 0.5, 0.3, 1, 1, 1, 1e32, 1.5, 0.0)
                m.view(np.uint32)[18:24] = (4, 0, 1, 5, 6 if mtype == SG else 7, 0)
                m.view(np.uint32)[19] = 9 + tex
            else:
                m.view(np.uint32)[20] = 9 + tex
            ids.append(mtype | (len(mats[mtype]) << 8))
            mats[mtype].append(m)
        self.soup.meshes["MaterialId"] = ids
        self.mats = {k: np.ascontiguousarray(np.stack(v), np.float32) for k, v in mats.items()}
        d = self.soup.desc
        d.metallicRoughnessMaterials, d.metallicRoughnessMaterialCount = self.mats[MR].ctypes.data, len(self.mats[MR])
        d.specularGlossinessMaterials, d.specularGlossinessMaterialCount = self.mats[SG].ctypes.data, len(self.mats[SG])
        d.phongMaterials, d.phongMaterialCount = self.mats[PHONG].ctypes.data, len(self.mats[PHONG])
        self.texels = [np.ascontiguousarray(t) for t in _alpha_textures()]
        self.table = (pkg.TextureDesc * len(self.texels))()
        for i, t in enumerate(self.texels):
            self.table[i] = pkg.TextureDesc(t.shape[1], t.shape[0], SRGB, 1, None if pending else t.ctypes.data)
        d.textures, d.textureCount = C.addressof(self.table), len(self.texels)
        d.textureMemoryBudget = ALPHA_SHARE * len(self.texels)
        self.desc = d

    def texture_desc(self, pkg, i):
        t = self.texels[i]
        return pkg.TextureDesc(t.shape[1], t.shape[0], SRGB, 1, t.ctypes.data)


def _alpha_rays():
    """Per slot 20 000 axis-parallel rays and 5 000 oblique ones (1 000 + 250 for the constant quad of slot 6), aimed inside
    the slot's quads.  Returns (rays for closest queries, the same with tmax short of the wall, slot of every ray)."""
    rng = np.random.default_rng(78)
    rays, slots = [], []
    for slot in range(SLOTS):
        na, no = (20000, 5000) if slot < 6 else (1000, 250)
        z = min(q[3] for q in QUADS if q[2] == slot)
        tx, ty = 3.0 * slot + rng.uniform(0.02, 1.98, na + no), rng.uniform(0.02, 1.98, na + no)
        o = np.stack([tx, ty, np.full(na + no, RAY_Z)], 1)
        o[na:, 0] += rng.uniform(-1.5, 1.5, no)
        o[na:, 1] += rng.uniform(-1.5, 1.5, no)
        o = o.astype(np.float32)
        dvec = np.stack([tx, ty, np.full(na + no, z)], 1) - o
        dvec[:na] = (0, 0, 1)
        dvec = (dvec / np.linalg.norm(dvec, axis=1, keepdims=True)).astype(np.float32)
        r = np.zeros((na + no, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 1e-5, dvec, 1e4
        rays.append(r)
        slots.append(np.full(na + no, slot))
    rays = np.concatenate(rays)
    shadow = rays.copy()
    shadow[:, 7] = np.float32(5.5) / rays[:, 6]   # the wall is at (1 - -5) / d_z
    return rays, shadow, np.concatenate(slots)


_alpha_cache = {}


def _alpha_scene_reference(level0_of_scaled=None):
    """What every ray must report, from the float64 reference: per ray the expected quad (-1 = the wall) of a closest query,
    the occlusion of a shadow query, and which rays are excused.  level0_of_scaled: the bytes of the budget-scaled texture as
    uploaded (read back by the caller; the reference's own blit when None)."""
    key = None if level0_of_scaled is None else level0_of_scaled.tobytes()
    if key in _alpha_cache:
        return _alpha_cache[key]
    texels = _alpha_textures()
    rays, shadow, slot = _alpha_rays()
    n = len(rays)
    alphas = []
    for i, t in enumerate(texels):
        a = t[..., 3].astype(np.int64)
        if i == 6:
            plan = ref.planned_extent(600, 4, SRGB, ALPHA_SHARE)
            assert plan["extent"] == (300, 2) and plan["halvings"] == 1 and not plan["final_blit"]
            a = ref.blit_step(t, SRGB, 300, 2)[1][..., 3] if level0_of_scaled is None else level0_of_scaled[..., 3]
        else:
            assert ref.planned_extent(t.shape[1], t.shape[0], SRGB, ALPHA_SHARE)["scale"] == 1
        alphas.append(a)
    t_hit = np.full((len(QUADS), n), np.inf)
    a64 = np.zeros((len(QUADS), n))
    exact_one = np.zeros((len(QUADS), n), bool)
    grazing = np.zeros((len(QUADS), n), bool)
    m_alpha = 0.0
    for q, (name, tex, qslot, z, uvr, mirrored, mtype, factor) in enumerate(QUADS):
        corners, uv = np.float64(_quad_corners(qslot, z)), np.float64(_quad_uv(uvr, mirrored))
        h, w = alphas[tex].shape
        for tri in ((0, 1, 2), (2, 3, 0)):
            inside, t, u, v = ref.barycentrics_f64(corners[list(tri)], rays)
            margin = np.minimum(np.minimum(u, v), 1 - u - v)
            # the quad's outline: the two edges of each triangle that are not the shared diagonal (which is u = 0 in both)
            outline = np.minimum(v, 1 - u - v)
            grazing[q] |= (np.abs(outline) < 1e-4) & (margin > -1e-3) & np.isfinite(t)
            new = inside & ~np.isfinite(t_hit[q])
            b = np.stack([1 - u - v, u, v], 1)
            uvs = uv[list(tri)]
            tu, tv = b @ uvs[:, 0], b @ uvs[:, 1]
            a, one = ref.alpha_at(alphas[tex] / 255.0, w, h, tu, tv, factor)
            b32 = np.stack([np.float32(1) - np.float32(u) - np.float32(v), np.float32(u), np.float32(v)], 1).astype(np.float32)
            uv32 = np.float32(uvs)
            tu32 = (uv32[0, 0] * b32[:, 0] + uv32[1, 0] * b32[:, 1] + uv32[2, 0] * b32[:, 2]).astype(np.float32)
            tv32 = (uv32[0, 1] * b32[:, 0] + uv32[1, 1] * b32[:, 1] + uv32[2, 1] * b32[:, 2]).astype(np.float32)
            a32, _ = ref.alpha_at((alphas[tex].astype(np.float32) / np.float32(255)), w, h, tu32, tv32, np.float32(factor))
            if new.any():
                m_alpha = max(m_alpha, float(np.abs(np.float64(a32[new]) - a[new]).max()))
            t_hit[q] = np.where(new, t, t_hit[q])
            a64[q] = np.where(new, a, a64[q])
            exact_one[q] = np.where(new, one & (factor == 1.0), exact_one[q])
    m_a = 8 * M_ALPHA
    hit = np.isfinite(t_hit)
    a_eff = np.where(exact_one, 1.0, a64)
    keep_closest, keep_shadow = hit & (a_eff >= ref.CLOSEST_THRESHOLD), hit & (a_eff >= ref.SHADOW_THRESHOLD)
    closest = np.where(keep_closest.any(axis=0), np.argmin(np.where(keep_closest, t_hit, np.inf), axis=0), -1)
    occluded = keep_shadow.any(axis=0)
    band_c = hit & (np.abs(a_eff - ref.CLOSEST_THRESHOLD) <= m_a) & (a_eff != ref.CLOSEST_THRESHOLD)
    band_s = hit & (np.abs(a_eff - ref.SHADOW_THRESHOLD) <= m_a) & (a_eff != ref.SHADOW_THRESHOLD)
    # what an excused closest ray may report besides `closest`: the nearest kept quad with every quad in the band kept, the
    # same with every quad in the band or grazed left out, or a quad it grazes
    nearest = lambda keep: np.where(keep.any(axis=0), np.argmin(np.where(keep, t_hit, np.inf), axis=0), -1)  # noqa: E731
    alternatives = np.stack([closest, nearest(keep_closest | band_c), nearest(keep_closest & ~band_c & ~grazing)])
    out = dict(rays=rays, shadow=shadow, slot=slot, closest=closest, occluded=occluded, excused_closest=(band_c | grazing).any(axis=0),
               excused_shadow=(band_s | grazing).any(axis=0), m_alpha=m_alpha, a=a_eff, hit=hit, alternatives=alternatives, grazing=grazing)
    _alpha_cache[key] = out
    return out


def _check_any_hit(want, closest_quad, occluded, label):
    """closest_quad: per ray the quad a closest query reported (-1 the wall, -2 a miss); occluded: the shadow query's flag."""
    slot = want["slot"]
    for s in range(SLOTS):
        sel = slot == s
        name = " + ".join(q[0] for q in QUADS if q[2] == s)
        for kind, got, exp, exc in (("closest", closest_quad, want["closest"], want["excused_closest"]), ("shadow", occluded, want["occluded"], want["excused_shadow"])):
            bad = sel & ~exc & (got != exp)
            assert not bad.any(), f"{label}, {name}, {kind}: {int(bad.sum())} of {int(sel.sum())} rays decided differently, first ray {int(np.flatnonzero(bad)[0])}: " \
                                  f"{got[np.flatnonzero(bad)[0]]} != {exp[np.flatnonzero(bad)[0]]}, alphas {want['a'][:, np.flatnonzero(bad)[0]]}"
            assert exc[sel].mean() <= 0.02, f"{label}, {name}, {kind}: {exc[sel].mean():.4f} of the rays excused"
    # an excused closest ray may only report one of the readings of the quads in the band or grazed: never another quad, never a miss
    exc = np.flatnonzero(want["excused_closest"])
    got = closest_quad[exc]
    allowed = (want["alternatives"][:, exc] == got).any(axis=0) | ((got >= 0) & want["grazing"][np.maximum(got, 0), exc])
    assert allowed.all(), f"{label}: {int((~allowed).sum())} excused rays report a quad that no reading of the band allows, first ray {exc[~allowed][:1]}"
    assert (closest_quad >= -1).all(), f"{label}: {int((closest_quad < -1).sum())} rays missed the wall"
    print(f"{label}: {len(exc)} closest and {int(want['excused_shadow'].sum())} shadow rays of {len(slot)} excused")


def _check_alpha_reference_outcomes(want):
    """The scene shows both outcomes of every decision it can (computed from the reference alone)."""
    slot, closest, occ = want["slot"], want["closest"], want["occluded"]
    for q, (name, tex, s, *_rest) in enumerate(QUADS):
        sel = slot == s
        share = float((closest[sel] == q).mean())
        if name == "1x1 x 0.6" or name.startswith("2x2"):   # a constant alpha above the threshold: always kept
            assert share == 1.0, name
        else:
            assert 0.05 <= share <= 0.95, (name, share)
        if name in ("37x21", "300x2"):
            assert 0.05 <= float(occ[sel].mean()) <= 0.95, name
    assert 0.05 <= float((closest[slot == 5] == -1).mean()) and 0.05 <= float(occ[slot == 5].mean()) <= 0.95
    # alpha <= 0.9 never stops a shadow ray; the 2 x 1 texture reaches 1 only on a set of measure zero; constants below 1
    for s in (2, 3, 4, 6):
        assert not occ[slot == s].any(), s
    assert (want["a"][2][want["hit"][2]] <= 0.9).all()
    # the exact-1 footprints exist and are decided, not excused
    assert ((want["a"] == 1.0) & want["hit"]).any(axis=0)[~want["excused_shadow"]].sum() > 5000
    # exactly 0.5: kept by a closest ray (alpha < 0.5 is false), and not excused
    assert (want["a"][7][want["hit"][7]] == 0.5).all() and not want["excused_closest"][slot == 6].any()


def test_alpha_reference_scene_shows_both_outcomes():
    want = _alpha_scene_reference()
    _check_alpha_reference_outcomes(want)
    # the recorded shares of excused rays: the worst slot, within a quarter of a percent of what was recorded, far below the cap
    for kind in ("closest", "shadow"):
        worst = max(float(want["excused_" + kind][want["slot"] == s].mean()) for s in range(SLOTS))
        print(f"excused {kind} rays, worst slot: {worst:.4f}")
        assert abs(worst - EXCUSED_RAYS[kind]) <= 0.0025 and worst <= 0.02
    # the vectorised barycentrics are util.moller_trumbore_f64's
    rays = want["rays"][::997]
    tri = np.float64(_quad_corners(0, -0.1))[[0, 1, 2]]
    inside, t, u, v = ref.barycentrics_f64(tri, rays)
    for k, r in enumerate(rays):
        i2, t2, u2, v2, _ = util.moller_trumbore_f64(tri[None], r)
        assert bool(i2[0]) == bool(inside[k]) and (not inside[k] or (t2[0] == t[k] and u2[0] == u[k] and v2[0] == v[k]))


def _scaled_alpha_level0(sample):
    """Level 0 of the budget-scaled 600 x 4 texture (scene texture 6) as uploaded, held to the reference's blit by the tie rule."""
    ys, xs = np.mgrid[0:2, 0:300]
    u, fu = _exact_factor(xs.reshape(-1) + 0.5, 300)
    v, fv = _exact_factor(ys.reshape(-1) + 0.5, 2)
    got = _to_bytes(sample(_inputs(9 + 6, u, v), True).view(np.float32).reshape(2, 300, 4), SRGB)
    vref, _ = ref.blit_step(_alpha_textures()[6], SRGB, 300, 2)
    _tie_rule(vref, got, SRGB, "600x4 -> 300x2")
    return got


def _oracle_quads(tri):
    return np.where(tri == 0xFFFFFFFF, -2, np.where(tri < 2, -1, (tri.astype(np.int64) - 2) // 2))


@pytest.mark.parametrize("brute", [False, True], ids=["tree", "brute-force"])
def test_oracle_any_hit_against_float64_alpha(pkg, orc, brute):
    scene = AlphaScene(pkg)
    osc = orc.OracleScene(scene.desc, build_bvh=not brute)
    want = _alpha_scene_reference(_scaled_alpha_level0(lambda inp, implicit: osc.test_texture(inp, implicit)))
    _check_alpha_reference_outcomes(want)
    got = osc.trace_closest(want["rays"], brute_force=brute)
    occ = osc.trace_any(want["shadow"], brute_force=brute)
    _check_any_hit(want, _oracle_quads(got["tri"]), occ != 0, "oracle")


# ---------------------------------------------------------------------------------------
# GPU: the kernels against the reference, not via the oracle
# ---------------------------------------------------------------------------------------
def _blocking_sampler(r, desc):
    r._check(r.lib.ptx_scene_upload(r.handle, C.byref(desc)))
    return lambda inp, implicit: r.test_texture(inp, implicit)


@pytest.fixture(scope="module")
def own_renderer(pkg):
    import torch  # noqa: F401

    r = pkg.Renderer()
    yield r
    r.close()


def _streamed_sampler(pkg, r, desc):
    table = (pkg.TextureDesc * desc.textureCount).from_address(desc.textures)
    full = [pkg.TextureDesc(t.width, t.height, t.format, t.levels, t.data) for t in table]
    pend = (pkg.TextureDesc * len(full))(*[pkg.TextureDesc(t.width, t.height, t.format, t.levels, None) for t in full])
    d = type(desc).from_buffer_copy(desc)
    d.textures = C.addressof(pend)
    r.upload_streamed(d, None, build=False)
    for i, t in enumerate(full):
        r.upload_texture(i, t)
    assert r.commit_textures() == len(full)
    return lambda inp, implicit: r.test_texture(inp, implicit)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CHAIN_CASES)), ids=[c[0] for c in CHAIN_CASES])
def test_chain_blocking_upload_against_float64_blit(pkg, gpu_renderer, base_scene, k):
    case = CHAIN_CASES[k]
    d, keep = _one_texture_desc(pkg, base_scene, *case[1:5])
    _check_chain(_blocking_sampler(gpu_renderer, d), case)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SCALED_CASES)), ids=[c[0] for c in SCALED_CASES])
def test_scaled_blocking_upload_against_float64_blit(pkg, gpu_renderer, base_scene, k):
    case = SCALED_CASES[k]
    d, keep = _one_texture_desc(pkg, base_scene, *case[1:5], budget=case[5])
    _check_scaled(_blocking_sampler(gpu_renderer, d), case)


@pytest.mark.gpu
def test_file_chain_under_a_budget_and_force_full_on_the_device(pkg, gpu_renderer, base_scene):
    _check_file_chain_and_force_full(pkg, base_scene, lambda d: _blocking_sampler(gpu_renderer, d))


@pytest.mark.gpu
def test_srgb_table_on_the_device(pkg, gpu_renderer, base_scene):
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 4, axis=2)
    d, keep = _one_texture_desc(pkg, base_scene, 256, 1, SRGB, ramp)
    got = _read_level(_blocking_sampler(gpu_renderer, d), 256, 1, 0, need_exact=True)[0]
    assert np.abs(got[:, :3] - ref.srgb_to_linear(np.arange(256) / 255.0)[:, None]).max() <= 8 * SRGB_TABLE_ERR
    assert np.abs(got[:, 3] - np.arange(256) / 255.0).max() <= 2.0 ** -24


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAMED)
def test_chain_streamed_upload_against_float64_blit(pkg, own_renderer, base_scene, name):
    """upload_streamed -> upload_texture -> commit_textures: the fused k_stream_chain path."""
    case = next(c for c in CHAIN_CASES if c[0] == name)
    d, keep = _one_texture_desc(pkg, base_scene, *case[1:5])
    _check_chain(_streamed_sampler(pkg, own_renderer, d), case)


def _gpu_any_hit(r, scene, want, label):
    hits, ids = r.trace_rays(want["rays"], any_hit=False)
    gid = util.global_ids(scene.desc, ids)
    occ, _ = r.trace_rays(want["shadow"], any_hit=True)
    _check_any_hit(want, _oracle_quads(gid), occ[:, 3] != 0, label)


def _refit(r):
    """A refit with unchanged instance transforms.  The tree of an upload keeps no build state, so the first update after it
    is a rebuild whatever is asked for (tests/test_animation.py does the same): rebuild explicitly, then refit."""
    identity = util.IDENTITY_3X4.reshape(1, 12)
    r.update_animation(instance_transforms=identity, rebuild=True)
    r.update_animation(instance_transforms=identity)


@pytest.mark.gpu
def test_any_hit_blocking_upload_against_float64_alpha(pkg):
    """Renderer.trace_rays on the hand-built scene after a blocking upload, and again after a refit with unchanged instance
    transforms, which rewrites the any-hit records (the scene has no animated geometry: the refit is by instance transform)."""
    import torch  # noqa: F401

    scene = AlphaScene(pkg)
    r = pkg.Renderer()
    r.upload(scene.desc)
    want = _alpha_scene_reference(_scaled_alpha_level0(lambda inp, implicit: r.test_texture(inp, implicit)))
    _gpu_any_hit(r, scene, want, "blocking")
    _refit(r)
    _gpu_any_hit(r, scene, want, "blocking, after a refit")
    r.close()


@pytest.mark.gpu
def test_any_hit_streamed_before_the_build_against_float64_alpha(pkg):
    import torch  # noqa: F401

    scene, pending = AlphaScene(pkg), AlphaScene(pkg, pending=True)
    r = pkg.Renderer()
    r.upload_streamed(pending.desc, None, build=False)
    for i in range(len(scene.texels)):
        r.upload_texture(i, scene.texture_desc(pkg, i))
    assert r.commit_textures() == len(scene.texels)
    r._check(r.lib.ptx_build_accel(r.handle))
    want = _alpha_scene_reference(_scaled_alpha_level0(lambda inp, implicit: r.test_texture(inp, implicit)))
    _gpu_any_hit(r, scene, want, "streamed")
    _refit(r)
    _gpu_any_hit(r, scene, want, "streamed, after a refit")
    r.close()
