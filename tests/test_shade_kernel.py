"""k_shade's resources and the BSDF it evaluates.

CPU: the kernel metadata of the built libptx_hip.so (the gfx950 code object's notes) -- the plain shade kernel keeps its
state in registers: no VGPR spills, no scratch, and none of the material sort's LDS.
GPU: evaluateBSDF and sampleBSDF through ptx_test_eval against the oracle bit for bit, on a dense grid over the branch
edges of the shared reflection terms (L.z at 0 and at 1e-5 +- 1 ulp, VdotH <= 0, V.z near 0, Metalness and Transmission
at 0 and 1, roughness 0.01)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import util


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def _kernel_metadata(lib, tmp_path):
    """{mangled kernel name: {metadata key: value}} of the gfx950 code object inside `lib`."""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    assert objcopy and bundler and readelf, "the ROCm LLVM tools that read a HIP fat binary are missing"
    fatbin, co = str(tmp_path / "fatbin.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fatbin, lib, os.devnull])
    subprocess.check_call([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fatbin, "--output=" + co])
    notes = subprocess.run([readelf, "--notes", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in notes.splitlines():
        if line.startswith("  - ."):  # a new entry of amdhsa.kernels
            cur = {}
        m = re.match(r"^\s{2}[- ] \.(\w+):\s+(\S+)\s*$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                kernels[m.group(2)] = cur
    return kernels


def test_plain_shade_kernel_keeps_its_state_in_registers(pkg, tmp_path):
    meta = _kernel_metadata(pkg.HIP_LIB, tmp_path)
    shade = {k: v for k, v in meta.items() if k.startswith("_Z7k_shadeILb0E")}
    assert len(shade) == 1, sorted(meta)
    (kd,) = shade.values()
    assert int(kd["vgpr_spill_count"]) == 0, kd
    assert int(kd["private_segment_fixed_size"]) == 0, kd  # no scratch
    # the material sort lives in k_shade_sorted: its 4 KiB of sorted slots are not allocated here
    assert int(kd["group_segment_fixed_size"]) < 1024, kd
    sorted_ = [v for k, v in meta.items() if k.startswith("_Z14k_shade_sortedILb0E")]
    assert len(sorted_) == 1 and int(sorted_[0]["group_segment_fixed_size"]) >= 4096


# ---------------------------------------------------------------------------------------
# GPU: the BSDF bit for bit
# ---------------------------------------------------------------------------------------
def _ulp_neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _bsdf_grid():
    """(materials, V, L): every combination of a few materials, view directions and light directions."""
    mats = []
    for color in ((0.8, 0.3, 0.1), (1.0, 1.0, 1.0)):
        for rough in (0.01, 0.1, 0.5, 1.0):
            for metal in (0.0, 0.5, 1.0):
                for trans in (0.0, 1.0):
                    for eta in (1.0 / 1.5, 1.5):
                        mats.append([*color, rough, metal, trans, eta, 0.0])
    mats = np.float32(mats)
    Vs = [_unit([0.3, -0.2, 1.0]), _unit([0.0, 0.0, 1.0]), _unit([0.9, 0.1, 0.05]), _unit([1.0, 0.0, 1e-4]),
          _unit([-0.5, 0.7, 0.4]), _unit([0.2, 0.1, -0.9])]
    Ls = []
    for z in [0.0, -0.0] + _ulp_neighbours(1e-5) + _ulp_neighbours(-1e-5) + [0.5, 1.0, -0.5, -1.0]:
        z = np.float32(z)
        r = np.sqrt(max(0.0, 1.0 - float(z) * float(z)))
        for phi in (0.0, 2.0, 4.0):
            Ls.append(np.float32([r * np.cos(phi), r * np.sin(phi), z]))
    for V in Vs[:3]:  # light directions behind V's half vector: V.H <= 0
        Ls.append(np.float32([-V[0], -V[1], np.float32(2e-5)]))
        Ls.append(_unit([-V[0] * 3.0, -V[1] * 3.0, 0.5]))
    return mats, np.float32(Vs), np.float32(Ls)


@pytest.mark.gpu
def test_evaluate_bsdf_matches_oracle_bitexact(pkg, orc, gpu_renderer):
    mats, Vs, Ls = _bsdf_grid()
    nm, nv, nl = len(mats), len(Vs), len(Ls)
    m = np.repeat(mats, nv * nl, axis=0)
    V = np.tile(np.repeat(Vs, nl, axis=0), (nm, 1))
    L = np.tile(Ls, (nm * nv, 1))
    inp = np.concatenate([m, V, L], axis=1).astype(np.float32)
    fn = pkg.FN["evaluateBSDF"]
    out = gpu_renderer.test_eval(fn, inp)
    ref = orc.test_eval(fn, inp, 4)
    ok = util.bits_equal_or_both_nan(out, ref)
    assert ok.all(), f"{int((~ok).any(axis=1).sum())} of {len(inp)} cases differ, first {inp[~ok.all(axis=1)][:3]}"
    # the grid reaches both sides of every edge it is meant to
    lz = L[:, 2]
    assert (lz == 0).any() and (lz == np.float32(1e-5)).any() and ((lz > 0) & (lz < np.float32(1e-5))).any()
    assert (out.view(np.float32)[:, 3] > 0).any() and (out.view(np.float32)[:, 3] == 0).any()


@pytest.mark.gpu
def test_sample_bsdf_matches_oracle_bitexact(pkg, orc, gpu_renderer):
    mats, Vs, _ = _bsdf_grid()
    seeds = np.arange(64, dtype=np.uint32) * np.uint32(2654435761)
    nm, nv, ns = len(mats), len(Vs), len(seeds)
    m = np.repeat(mats, nv * ns, axis=0)
    V = np.tile(np.repeat(Vs, ns, axis=0), (nm, 1))
    s = np.tile(seeds, nm * nv).reshape(-1, 1)
    inp = np.concatenate([m.view(np.uint32), V.view(np.uint32), s], axis=1)
    fn = pkg.FN["sampleBSDF"]
    out = gpu_renderer.test_eval(fn, inp)
    ref = orc.test_eval(fn, inp, 8)
    assert (out[:, 7] == ref[:, 7]).all()  # the RNG state
    ok = util.bits_equal_or_both_nan(out, ref)
    assert ok.all(), f"{int((~ok).any(axis=1).sum())} of {len(inp)} cases differ"
