"""The words packed into the path state's records (csrc/pt_path_words.hpp): the state word bounce | smpl << 16 and the dead-slot
pattern, the shadow length with the "path ends" flag in its sign bit, the shadow result byte.

Without a GPU: the header as a stand-alone host program, plain and under the address / undefined-behaviour sanitizers.  The program
walks the whole state-word grid itself and prints what it packed; the bit patterns it prints are checked here against struct's.
The records that carry these words are held bit for bit by tests/test_path_state_layout.py on the GPU."""
import os
import struct
import subprocess

import pytest

SAMPLES = [0, 1, 0x1234, 0x7FFF, 0x8000, 0xFFFE]  # 0xfffe: the largest a launch stores (SampleCount <= 0xffff)
DEAD_WORD = 0xFFFFFFFF
# the smallest denormal, tmin of every ray, a light distance, the directional light's 100000, +inf
LENGTHS = [struct.unpack("<f", struct.pack("<I", 1))[0], 1e-5, 7.25, 100000.0, float("inf")]

_PROGRAM = r"""
#include "pt_path_words.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
static_assert(kMaxSampleCount == 0xffffu && kMaxBounceCount == 0xffffu, "16 bits each");
static_assert(packState(0u, 0u) == 0u, "first bounce of the first sample: the state at which rad is not read");
static_assert(kShadowLightVisible == 1u && kShadowEndsPath == 2u, "the result byte");
static_assert(kDeadPair != kMissPair, "a dead slot is not shaded as a miss");
int main(int argc, char **argv) // sample indices, then "--", then shadow lengths as bit patterns
{
    int i = 1;
    unsigned long bad = 0, words = 0;
    for (; i < argc && std::strcmp(argv[i], "--") != 0; i++)
    {
        const uint32_t smpl = (uint32_t)strtoul(argv[i], nullptr, 0);
        for (uint32_t bounce = 0; bounce <= kMaxBounceCount; bounce++)
        {
            const uint32_t w = packState(bounce, smpl);
            words++;
            bad += stateBounce(w) != bounce || stateSample(w) != smpl || w == kDeadWord;
            const uint32_t other = withBounce(w, kMaxBounceCount - bounce);
            bad += stateSample(other) != smpl || stateBounce(other) != kMaxBounceCount - bounce;
        }
        printf("state %u %u %u\n", smpl, packState(0u, smpl), packState(kMaxBounceCount, smpl));
    }
    printf("words %lu bad %lu dead %u\n", words, bad, kDeadWord);
    for (i++; i < argc; i++)
        for (int flag = 0; flag < 2; flag++)
        {
            const uint32_t bits = (uint32_t)strtoul(argv[i], nullptr, 0);
            const uint32_t w = packShadowLength(bitsFloat(bits), flag != 0);
            printf("length %u %d %u %u %d\n", bits, flag, w, floatBits(shadowLength(w)), shadowEndsPath(w) ? 1 : 0);
        }
    for (int occluded = 0; occluded < 2; occluded++)
        for (int ends = 0; ends < 2; ends++)
        {
            const uint32_t b = packShadowResult(occluded != 0, ends != 0);
            printf("result %d %d %u %d %d\n", occluded, ends, b, (b & kShadowLightVisible) ? 1 : 0, (b & kShadowEndsPath) ? 1 : 0);
        }
    return bad ? 1 : 0;
}
"""


def _bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_path_words_header_alone_round_trips_every_word(pkg, tmp_path, flags):
    """pt_path_words.hpp compiles with the host compiler and nothing else.  packState round-trips for every bounce in [0, 65535] at
    each sample index of SAMPLES, no such word is kDeadWord and withBounce keeps the sample half; shadowLength returns the bits of
    every length of LENGTHS under both flag values and shadowEndsPath the flag; the four result bytes round-trip."""
    src, exe = tmp_path / "words.cpp", tmp_path / "words"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(pkg.PKG_DIR, "csrc"), str(src), "-o", str(exe)])
    args = [str(s) for s in SAMPLES] + ["--"] + [str(_bits(d)) for d in LENGTHS]
    done = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr, (done.stdout[-400:], done.stderr)
    rows = [line.split() for line in done.stdout.split("\n")[:-1]]
    states = [[int(x) for x in r[1:]] for r in rows if r[0] == "state"]
    assert states == [[s, s << 16, s << 16 | 0xFFFF] for s in SAMPLES]
    assert all(w != DEAD_WORD for s in states for w in s[1:])
    assert [r for r in rows if r[0] == "words"] == [["words", str(65536 * len(SAMPLES)), "bad", "0", "dead", str(DEAD_WORD)]]
    lengths = [[int(x) for x in r[1:]] for r in rows if r[0] == "length"]
    assert lengths == [[_bits(d), f, _bits(d) | f << 31, _bits(d), f] for d in LENGTHS for f in (0, 1)]
    results = [[int(x) for x in r[1:]] for r in rows if r[0] == "result"]
    assert results == [[o, e, (1 - o) | e << 1, 1 - o, e] for o in (0, 1) for e in (0, 1)]
