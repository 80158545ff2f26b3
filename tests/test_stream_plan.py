"""csrc/pt_stream_plan.hpp: which streams a launch uses is one pure function of (hardware queues granted, live handles, what the
handle asked for).  tests/stream_plan_check.cpp checks it over queues 1..32 x handles 1..20 x the flag x PTX_STREAM_PLAN as a
program of its own, built with the address and undefined-behaviour sanitizers: two streams whenever everything fits, never for a
handle that asked for one, monotone in the queue count."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path-tracing_amd", "csrc")


def test_plan_properties_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing about it depends on how it is loaded
                    "-I", CSRC, "-o", exe, os.path.join(HERE, "stream_plan_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout
    assert p.stdout.strip().splitlines()[-1].startswith("ok:"), p.stdout


def test_the_header_has_no_hip_in_it():
    text = open(os.path.join(CSRC, "pt_stream_plan.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>"], includes
