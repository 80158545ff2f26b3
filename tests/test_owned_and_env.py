"""The two HIP-free headers a handle is made of before it touches the device: csrc/pt_owned.hpp (Owned: the one owner of every event,
stream and page-locked block of the handle) and csrc/pt_env.hpp (EnvSwitches::read, the only reader of the library's environment
switches).

Both are compiled alone, with the host compiler, into stand-alone programs, plain and under the address / undefined-behaviour
sanitizers, and run as their own executables.

EXPECTED below was not derived from the reader under test: before EnvSwitches moved to pt_env.hpp and its read() was rewritten around
four helpers, the struct was lifted verbatim out of pt_runtime.hpp into a program with the `main` of _ENV_PROGRAM, run over this
table of environments, and what it printed is recorded here (DEFAULTS: the fields with nothing set; per case the fields that differ)."""
import os
import subprocess

import pytest

FLAGS = [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]]


def _compile(pkg, tmp_path, name, text, flags):
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(text)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(pkg.PKG_DIR, "csrc"), str(src), "-o", str(exe)])
    return str(exe)


# =====================================================================================================
# pt_owned.hpp
# =====================================================================================================

_OWNED_PROGRAM = r"""
#include "pt_owned.hpp"
#include <cstdio>
#include <vector>
// An int handle (0 = empty) and a Destroy that counts its calls per handle value.  Every case uses values of its own; at the end
// every adopted value was destroyed exactly once, and no borrowed value and no empty owner ever reached Destroy.
static int g_destroyed[64];
static void destroy(int h) { g_destroyed[h]++; }
using Own = Owned<int, destroy>;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); g_failed = 1; } } while (0)
int main()
{
    { Own e; CHECK(!e); CHECK(e.get() == 0); e.release(); Own f(std::move(e)); Own g; g = std::move(f); } // empty owners
    { Own a; a.adopt(1); CHECK(a); CHECK(a.get() == 1); CHECK(g_destroyed[1] == 0); } // construct / destruct
    CHECK(g_destroyed[1] == 1);
    { Own a; a.adopt(2); a.release(); CHECK(!a); CHECK(a.get() == 0); CHECK(g_destroyed[2] == 1); a.release(); CHECK(g_destroyed[2] == 1); } // release() twice
    CHECK(g_destroyed[2] == 1);
    { Own a; a.adopt(3); Own b(std::move(a)); CHECK(!a); CHECK(b.get() == 3); CHECK(g_destroyed[3] == 0); } // move-construct
    CHECK(g_destroyed[3] == 1);
    { // move-assign onto a non-empty owner: the target's handle goes, the source is left empty
        Own a, b; a.adopt(4); b.adopt(5); b = std::move(a);
        CHECK(g_destroyed[5] == 1); CHECK(g_destroyed[4] == 0); CHECK(!a); CHECK(b.get() == 4);
    }
    CHECK(g_destroyed[4] == 1); CHECK(g_destroyed[5] == 1);
    { Own a; a.adopt(6); Own &same = a; a = std::move(same); CHECK(a.get() == 6); CHECK(g_destroyed[6] == 0); } // self-move-assign
    CHECK(g_destroyed[6] == 1);
    { // a vector of owners growing past several reallocations, then cleared
        std::vector<Own> v;
        for (int h = 10; h < 30; h++) { Own o; o.adopt(h); v.push_back(std::move(o)); }
        for (int h = 10; h < 30; h++) { CHECK(v[h - 10].get() == h); CHECK(g_destroyed[h] == 0); }
        v.clear();
        for (int h = 10; h < 30; h++) CHECK(g_destroyed[h] == 1);
    }
    { // borrow(): held, moved about, released, assigned over -- never destroyed; and it releases what the owner held before
        Own a; a.borrow(40); CHECK(a); CHECK(a.get() == 40);
        Own b(std::move(a)); CHECK(!a); Own c; c = std::move(b); CHECK(c.get() == 40); c.release(); CHECK(!c);
        Own d; d.borrow(41);
        Own e; e.adopt(42); e.borrow(43); CHECK(g_destroyed[42] == 1); CHECK(e.get() == 43);
        Own f; f.borrow(44); f.adopt(45); CHECK(f.get() == 45); // (and the other way round)
        Own g; g.adopt(46); g.adopt(47); CHECK(g_destroyed[46] == 1);
    }
    for (int h = 0; h < 64; h++)
    {
        const bool adopted = (h >= 1 && h <= 6) || (h >= 10 && h < 30) || h == 42 || h == 45 || h == 46 || h == 47;
        if (g_destroyed[h] != (adopted ? 1 : 0)) { printf("handle %d destroyed %d times\n", h, g_destroyed[h]); g_failed = 1; }
    }
    if (!g_failed) printf("ok\n");
    return g_failed;
}
"""


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "asan-ubsan"])
def test_owned_destroys_every_adopted_handle_once_and_no_borrowed_one(pkg, tmp_path, flags):
    """construct / destruct, release() twice, move-construct, move-assign onto a non-empty owner, self-move-assign, a vector of owners
    past a reallocation and cleared, borrow(): every adopted value reaches Destroy exactly once, no borrowed and no empty one does"""
    exe = _compile(pkg, tmp_path, "owned", _OWNED_PROGRAM, flags)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert (done.returncode, done.stdout, done.stderr) == (0, "ok\n", ""), (done.stdout[-2000:], done.stderr[-2000:])


def test_the_two_headers_have_no_hip_in_them(pkg):
    def includes(name):
        text = open(os.path.join(pkg.PKG_DIR, "csrc", name)).read()
        return sorted(line.split()[1] for line in text.splitlines() if line.startswith("#include"))

    assert includes("pt_owned.hpp") == ["<utility>"]
    assert includes("pt_env.hpp") == ["<algorithm>", "<cstdint>", "<cstdlib>", "<cstring>"]


# =====================================================================================================
# pt_env.hpp
# =====================================================================================================

_ENV_PROGRAM = r"""
#include "pt_env.hpp"
#include <cstdio>
// every field of EnvSwitches::read(), one "name=value" per line
int main()
{
    const EnvSwitches e = EnvSwitches::read();
    printf("cuPartition=%u\n", e.cuPartition);
    printf("singleStream=%d\n", (int)e.singleStream);
    printf("verbose=%d\n", (int)e.verbose);
    printf("karrasBuilder=%d\n", (int)e.karrasBuilder);
    printf("plocFixed=%d\n", (int)e.plocFixed);
    printf("plocRadius=%u\n", e.plocRadius);
    printf("plocShape=%.9g\n", (double)e.plocShape);
    printf("reinsertPasses=%d\n", e.reinsertPasses);
    printf("splitBudget=%.9g\n", (double)e.splitBudget);
    printf("layout=%d\n", e.layout);
    printf("collapse=%d\n", e.collapse);
    printf("shadeSort=%d\n", e.shadeSort);
    printf("tailThreshold=%ld\n", e.tailThreshold);
    printf("framesPerWave=%u\n", e.framesPerWave);
    printf("raysPerThread=%u\n", e.raysPerThread);
    printf("residentCap=%ld\n", e.residentCap);
    printf("copyGroups=%u\n", e.copyGroups);
    printf("snapshotMemcpy=%d\n", (int)e.snapshotMemcpy);
    printf("fenceRefit=%d\n", (int)e.fenceRefit);
    printf("pairLeaves=%d\n", (int)e.pairLeaves);
    printf("firstBounce=%d\n", (int)e.firstBounce);
    printf("streamLevelwise=%d\n", (int)e.streamLevelwise);
    printf("streamPlan=%d\n", (int)e.streamPlan);
    printf("bcRowMapping=%d\n", (int)e.bcRowMapping);
    printf("copyRuntime=%d\n", (int)e.copyRuntime);
    return 0;
}
"""

# what the reader of the commit before printed with none of the variables set ...
DEFAULTS = {
    'cuPartition': '0', 'singleStream': '0', 'verbose': '0', 'karrasBuilder': '0', 'plocFixed': '0', 'plocRadius': '0', 'plocShape': '0',
    'reinsertPasses': '-1', 'splitBudget': '-1', 'layout': '-1', 'collapse': '-1', 'shadeSort': '-1', 'tailThreshold': '-1', 'framesPerWave': '8',
    'raysPerThread': '0', 'residentCap': '-1', 'copyGroups': '0', 'snapshotMemcpy': '0', 'fenceRefit': '0', 'pairLeaves': '1', 'firstBounce': '1',
    'streamLevelwise': '0', 'streamPlan': '1', 'bcRowMapping': '0', 'copyRuntime': '0',
}
# ... and under each environment: (the variables set, the fields that differ from DEFAULTS).  Every boolean variable as "", 0, 1,
# yes; the two words and another word each; every number as 0, 7, -3, abc, 2.5; PTX_PLOC_SHAPE alone, PTX_PLOC_RADIUS=0 alone, both.
EXPECTED = [
    ({'PTX_VERBOSE': ''}, {'verbose': '1'}),
    ({'PTX_VERBOSE': '0'}, {'verbose': '1'}),
    ({'PTX_VERBOSE': '1'}, {'verbose': '1'}),
    ({'PTX_VERBOSE': 'yes'}, {'verbose': '1'}),
    ({'PTX_STREAM_LEVELWISE': ''}, {'streamLevelwise': '1'}),
    ({'PTX_STREAM_LEVELWISE': '0'}, {}),
    ({'PTX_STREAM_LEVELWISE': '1'}, {'streamLevelwise': '1'}),
    ({'PTX_STREAM_LEVELWISE': 'yes'}, {'streamLevelwise': '1'}),
    ({'PTX_COPY_RUNTIME': ''}, {'copyRuntime': '1'}),
    ({'PTX_COPY_RUNTIME': '0'}, {}),
    ({'PTX_COPY_RUNTIME': '1'}, {'copyRuntime': '1'}),
    ({'PTX_COPY_RUNTIME': 'yes'}, {'copyRuntime': '1'}),
    ({'PTX_SNAPSHOT_MEMCPY': ''}, {'snapshotMemcpy': '1'}),
    ({'PTX_SNAPSHOT_MEMCPY': '0'}, {}),
    ({'PTX_SNAPSHOT_MEMCPY': '1'}, {'snapshotMemcpy': '1'}),
    ({'PTX_SNAPSHOT_MEMCPY': 'yes'}, {'snapshotMemcpy': '1'}),
    ({'PTX_FENCE_REFIT': ''}, {'fenceRefit': '1'}),
    ({'PTX_FENCE_REFIT': '0'}, {}),
    ({'PTX_FENCE_REFIT': '1'}, {'fenceRefit': '1'}),
    ({'PTX_FENCE_REFIT': 'yes'}, {'fenceRefit': '1'}),
    ({'PTX_SINGLE_STREAM': ''}, {'singleStream': '1'}),
    ({'PTX_SINGLE_STREAM': '0'}, {}),
    ({'PTX_SINGLE_STREAM': '1'}, {'singleStream': '1'}),
    ({'PTX_SINGLE_STREAM': 'yes'}, {'singleStream': '1'}),
    ({'PTX_PAIR_LEAVES': ''}, {}),
    ({'PTX_PAIR_LEAVES': '0'}, {'pairLeaves': '0'}),
    ({'PTX_PAIR_LEAVES': '1'}, {}),
    ({'PTX_PAIR_LEAVES': 'yes'}, {}),
    ({'PTX_FIRST_BOUNCE': ''}, {}),
    ({'PTX_FIRST_BOUNCE': '0'}, {'firstBounce': '0'}),
    ({'PTX_FIRST_BOUNCE': '1'}, {}),
    ({'PTX_FIRST_BOUNCE': 'yes'}, {}),
    ({'PTX_STREAM_PLAN': ''}, {}),
    ({'PTX_STREAM_PLAN': '0'}, {'streamPlan': '0'}),
    ({'PTX_STREAM_PLAN': '1'}, {}),
    ({'PTX_STREAM_PLAN': 'yes'}, {}),
    ({'PTX_BC_MAPPING': 'rows'}, {'bcRowMapping': '1'}),
    ({'PTX_BC_MAPPING': 'cols'}, {}),
    ({'PTX_BUILDER': 'lbvh'}, {'karrasBuilder': '1'}),
    ({'PTX_BUILDER': 'ploc'}, {}),
    ({'PTX_COPY_GROUPS': '0'}, {}),
    ({'PTX_COPY_GROUPS': '7'}, {'copyGroups': '7'}),
    ({'PTX_COPY_GROUPS': '-3'}, {'copyGroups': '4294967293'}),
    ({'PTX_COPY_GROUPS': 'abc'}, {}),
    ({'PTX_COPY_GROUPS': '2.5'}, {'copyGroups': '2'}),
    ({'PTX_PLOC_SHAPE': '0'}, {'plocFixed': '1'}),
    ({'PTX_PLOC_SHAPE': '7'}, {'plocFixed': '1', 'plocShape': '7'}),
    ({'PTX_PLOC_SHAPE': '-3'}, {'plocFixed': '1', 'plocShape': '-3'}),
    ({'PTX_PLOC_SHAPE': 'abc'}, {'plocFixed': '1'}),
    ({'PTX_PLOC_SHAPE': '2.5'}, {'plocFixed': '1', 'plocShape': '2.5'}),
    ({'PTX_PLOC_RADIUS': '0'}, {'plocFixed': '1', 'plocRadius': '1'}),
    ({'PTX_PLOC_RADIUS': '7'}, {'plocFixed': '1', 'plocRadius': '7'}),
    ({'PTX_PLOC_RADIUS': '-3'}, {'plocFixed': '1', 'plocRadius': '4294967293'}),
    ({'PTX_PLOC_RADIUS': 'abc'}, {'plocFixed': '1', 'plocRadius': '1'}),
    ({'PTX_PLOC_RADIUS': '2.5'}, {'plocFixed': '1', 'plocRadius': '2'}),
    ({'PTX_REINSERT': '0'}, {'reinsertPasses': '0'}),
    ({'PTX_REINSERT': '7'}, {'reinsertPasses': '7'}),
    ({'PTX_REINSERT': '-3'}, {'reinsertPasses': '-3'}),
    ({'PTX_REINSERT': 'abc'}, {'reinsertPasses': '0'}),
    ({'PTX_REINSERT': '2.5'}, {'reinsertPasses': '2'}),
    ({'PTX_SPLIT_BUDGET': '0'}, {'splitBudget': '0'}),
    ({'PTX_SPLIT_BUDGET': '7'}, {'splitBudget': '7'}),
    ({'PTX_SPLIT_BUDGET': '-3'}, {'splitBudget': '-3'}),
    ({'PTX_SPLIT_BUDGET': 'abc'}, {'splitBudget': '0'}),
    ({'PTX_SPLIT_BUDGET': '2.5'}, {'splitBudget': '2.5'}),
    ({'PTX_NODE_LAYOUT': '0'}, {'layout': '0'}),
    ({'PTX_NODE_LAYOUT': '7'}, {'layout': '1'}),
    ({'PTX_NODE_LAYOUT': '-3'}, {'layout': '1'}),
    ({'PTX_NODE_LAYOUT': 'abc'}, {'layout': '0'}),
    ({'PTX_NODE_LAYOUT': '2.5'}, {'layout': '1'}),
    ({'PTX_COLLAPSE': '0'}, {'collapse': '0'}),
    ({'PTX_COLLAPSE': '7'}, {'collapse': '1'}),
    ({'PTX_COLLAPSE': '-3'}, {'collapse': '1'}),
    ({'PTX_COLLAPSE': 'abc'}, {'collapse': '0'}),
    ({'PTX_COLLAPSE': '2.5'}, {'collapse': '1'}),
    ({'PTX_SHADE_SORT': '0'}, {'shadeSort': '0'}),
    ({'PTX_SHADE_SORT': '7'}, {'shadeSort': '1'}),
    ({'PTX_SHADE_SORT': '-3'}, {'shadeSort': '1'}),
    ({'PTX_SHADE_SORT': 'abc'}, {'shadeSort': '0'}),
    ({'PTX_SHADE_SORT': '2.5'}, {'shadeSort': '1'}),
    ({'PTX_TAIL_THRESHOLD': '0'}, {'tailThreshold': '0'}),
    ({'PTX_TAIL_THRESHOLD': '7'}, {'tailThreshold': '7'}),
    ({'PTX_TAIL_THRESHOLD': '-3'}, {'tailThreshold': '-3'}),
    ({'PTX_TAIL_THRESHOLD': 'abc'}, {'tailThreshold': '0'}),
    ({'PTX_TAIL_THRESHOLD': '2.5'}, {'tailThreshold': '2'}),
    ({'PTX_FRAMES_PER_WAVE': '0'}, {'framesPerWave': '0'}),
    ({'PTX_FRAMES_PER_WAVE': '7'}, {'framesPerWave': '7'}),
    ({'PTX_FRAMES_PER_WAVE': '-3'}, {'framesPerWave': '4294967293'}),
    ({'PTX_FRAMES_PER_WAVE': 'abc'}, {'framesPerWave': '0'}),
    ({'PTX_FRAMES_PER_WAVE': '2.5'}, {'framesPerWave': '2'}),
    ({'PTX_RAYS_PER_THREAD': '0'}, {'raysPerThread': '1'}),
    ({'PTX_RAYS_PER_THREAD': '7'}, {'raysPerThread': '7'}),
    ({'PTX_RAYS_PER_THREAD': '-3'}, {'raysPerThread': '4294967293'}),
    ({'PTX_RAYS_PER_THREAD': 'abc'}, {'raysPerThread': '1'}),
    ({'PTX_RAYS_PER_THREAD': '2.5'}, {'raysPerThread': '2'}),
    ({'PTX_RESIDENT_CAP': '0'}, {'residentCap': '0'}),
    ({'PTX_RESIDENT_CAP': '7'}, {'residentCap': '7'}),
    ({'PTX_RESIDENT_CAP': '-3'}, {'residentCap': '-3'}),
    ({'PTX_RESIDENT_CAP': 'abc'}, {'residentCap': '0'}),
    ({'PTX_RESIDENT_CAP': '2.5'}, {'residentCap': '2'}),
    ({'PTX_CU_PARTITION': '0'}, {}),
    ({'PTX_CU_PARTITION': '7'}, {'cuPartition': '7'}),
    ({'PTX_CU_PARTITION': '-3'}, {'cuPartition': '4294967293'}),
    ({'PTX_CU_PARTITION': 'abc'}, {}),
    ({'PTX_CU_PARTITION': '2.5'}, {'cuPartition': '2'}),
    ({'PTX_PLOC_SHAPE': '0.5'}, {'plocFixed': '1', 'plocShape': '0.5'}),
    ({'PTX_PLOC_RADIUS': '0'}, {'plocFixed': '1', 'plocRadius': '1'}),
    ({'PTX_PLOC_SHAPE': '0.5', 'PTX_PLOC_RADIUS': '0'}, {'plocFixed': '1', 'plocRadius': '1', 'plocShape': '0.5'}),
]

BOOLEANS = ["PTX_VERBOSE", "PTX_STREAM_LEVELWISE", "PTX_COPY_RUNTIME", "PTX_SNAPSHOT_MEMCPY", "PTX_FENCE_REFIT", "PTX_SINGLE_STREAM", "PTX_PAIR_LEAVES",
            "PTX_FIRST_BOUNCE", "PTX_STREAM_PLAN"]
NUMBERS = ["PTX_COPY_GROUPS", "PTX_PLOC_SHAPE", "PTX_PLOC_RADIUS", "PTX_REINSERT", "PTX_SPLIT_BUDGET", "PTX_NODE_LAYOUT", "PTX_COLLAPSE", "PTX_SHADE_SORT",
           "PTX_TAIL_THRESHOLD", "PTX_FRAMES_PER_WAVE", "PTX_RAYS_PER_THREAD", "PTX_RESIDENT_CAP", "PTX_CU_PARTITION"]


def test_the_table_covers_every_variable_the_reader_names(pkg):
    """EXPECTED has the cases it claims, and pt_env.hpp reads no variable the table does not set"""
    import re

    want = [{name: v} for name in BOOLEANS for v in ("", "0", "1", "yes")]
    want += [{"PTX_BC_MAPPING": v} for v in ("rows", "cols")] + [{"PTX_BUILDER": v} for v in ("lbvh", "ploc")]
    want += [{name: v} for name in NUMBERS for v in ("0", "7", "-3", "abc", "2.5")]
    want += [{"PTX_PLOC_SHAPE": "0.5"}, {"PTX_PLOC_RADIUS": "0"}, {"PTX_PLOC_SHAPE": "0.5", "PTX_PLOC_RADIUS": "0"}]
    assert [env for env, _ in EXPECTED] == want
    text = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_env.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert set(re.findall(r'"(PTX_[A-Z_]+)"', code)) == set(BOOLEANS + NUMBERS + ["PTX_BC_MAPPING", "PTX_BUILDER"])


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "asan-ubsan"])
def test_env_switches_read_what_the_reader_before_read(pkg, tmp_path, flags):
    """every field of EnvSwitches::read() under every environment of the table is what the reader of the commit before printed"""
    exe = _compile(pkg, tmp_path, "env", _ENV_PROGRAM, flags)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PTX_")}

    def fields(env):
        done = subprocess.run([exe], env={**clean, **env}, capture_output=True, text=True, timeout=60)
        assert done.returncode == 0 and not done.stderr, (env, done.stderr[-2000:])
        return dict(line.split("=", 1) for line in done.stdout.splitlines())

    assert fields({}) == DEFAULTS
    for env, differs in EXPECTED:
        assert fields(env) == {**DEFAULTS, **differs}, env
