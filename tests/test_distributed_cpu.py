"""N > 1 path on CPU: two gloo ranks render their pixel-tile shards (with the oracle standing in
for the GPU renderer, which is absent here), exchange them with the same pack -> all_gather ->
unpack sequence bench.py uses, and rank 0 must hold the exact single-process frame."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from util import pack_shard as _pack, unpack_shard as _unpack

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, outdir):
    sys.path.insert(0, REPO)
    import __graft_entry__ as graft

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg, orc = graft.load_package(), graft.load_oracle()
    W, H, tile = 100, 70, 32
    s = pkg.Scene("default")
    osc = orc.OracleScene(s.desc)
    acc = np.zeros((H, W, 4), np.float32)
    shard = pkg.TileShard(rank, world, tile)
    for f in range(2):
        osc.render(s.uniform(W, H, bounces=4, total_samples=f), s.lights, W, H, accum=acc, shard=shard, threads=2)
    tiles = [pkg.owned_tiles(W, H, r, world, tile) for r in range(world)]
    n_max = max(len(t) for t in tiles)
    send = torch.zeros(n_max * tile * tile * 4)
    mine = _pack(acc, tiles[rank], tile, W, H)
    send[: mine.size] = torch.from_numpy(mine.reshape(-1))
    recv = torch.zeros(world * send.numel())
    dist.all_gather_into_tensor(recv, send)
    if rank == 0:
        full = np.zeros((H, W, 4), np.float32)
        for r in range(world):
            part = recv[r * send.numel():(r + 1) * send.numel()].numpy()[: len(tiles[r]) * tile * tile * 4]
            _unpack(part.reshape(len(tiles[r]), tile * tile, 4), tiles[r], tile, W, H, full)
        np.save(os.path.join(outdir, "gathered.npy"), full)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_tile_shard_gather(tmp_path, pkg, orc):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = np.load(tmp_path / "gathered.npy")
    W, H = 100, 70
    s = pkg.Scene("default")
    osc = orc.OracleScene(s.desc)
    ref = np.zeros((H, W, 4), np.float32)
    for f in range(2):
        osc.render(s.uniform(W, H, bounces=4, total_samples=f), s.lights, W, H, accum=ref)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def _frame_store_worker(rank, world, port, outdir):
    sys.path.insert(0, REPO)
    import bench

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    F, H, W = 3, 5, 7
    L = F * world // math.gcd(F, world)
    owned = [j for j in range(L) if j % world == rank]
    store = bench.FrameStore(torch, dist, L, H * W * 16, rank, world, owned, register=False)
    dist.barrier()  # (rank 0 unlinks the name right after the constructor's last barrier)
    assert store.shared and not os.path.exists(f"/dev/shm/ptx_frames_{port}_{os.getuid()}")  # unlinked once every rank has mapped it
    for j in owned:  # what a rank's gather launch does through the registered alias: it writes the frames it owns
        store.image(j, H, W)[...] = np.float32(100 * rank + j)
    dist.barrier()
    got = np.stack([store.image(j, H, W).copy() for j in range(L)])  # every rank sees every frame, whoever wrote it
    want = np.stack([np.full((H, W, 4), 100 * (j % world) + j, np.float32) for j in range(L)])
    assert (got == want).all()
    assert store.ptr(1) - store.ptr(0) == store.stride and store.stride % 4096 == 0
    dist.barrier()
    store.close()
    if rank == 0:
        np.save(os.path.join(outdir, "frames_seen_by_rank0.npy"), got)
    dist.destroy_process_group()


def test_host_frames_in_shared_memory_are_seen_by_every_rank(tmp_path):
    """bench.py's FrameStore for N > 1: ONE POSIX shared-memory segment of lcm(ranks, frames in flight) host
    frames that every rank maps; step k's frame lives at index k % L and is written by its owner, rank k % N; any process of the
    node reads every frame.  Two gloo ranks, no GPU (the hipHostRegister of the owned frames is the GPU tests' business): each
    writes the frames it owns, both read all six; the segment's name is gone from /dev/shm as soon as both have mapped it."""
    world = 2
    mp.spawn(_frame_store_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = np.load(tmp_path / "frames_seen_by_rank0.npy")
    assert got.shape == (6, 5, 7, 4) and [float(got[j, 0, 0, 0]) for j in range(6)] == [0.0, 101.0, 2.0, 103.0, 4.0, 105.0]


# ---------------------------------------------------------------------------------------
# the real N > 1 path: bench.py under torch.distributed.run, two ranks sharing GPU 0
# ---------------------------------------------------------------------------------------
def _run_bench_two_ranks(tmp_path, backend, extra=(), launcher=True, ranks=2):
    import json
    import subprocess

    out = tmp_path / f"gathered_{backend}.npy"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN")  # WARN: RCCL says WHY it refuses a communicator
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable]
    if launcher:  # as the driver starts an N > 1 run
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port", str(_free_port())]
    cmd += [os.path.join(REPO, "bench.py"), "--gpus", str(ranks), "--single-device", "--dist-backend", backend, "--full",
            "--steps", "2", "--warmup", "1", "--repeats", "1", "--scene", "chess_like", "--detail", "0.05", "--width", "328", "--height", "200",
            "--spp", "4", "--depth", "6", "--cpu-seconds", "1", "--dump-image", str(out), "--dump-frames", str(tmp_path / f"frames_{backend}.npy"), *extra]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    return p, out


def _single_rank_frame(pkg, W=328, H=200):
    scene = pkg.Scene("chess_like", 0.05)
    r = pkg.Renderer()
    r.upload(scene)
    r.resize(W, H)
    r.render_frames(scene.uniform(W, H, bounces=6), scene.lights, 0, 4)
    ref = r.readback()
    r.close()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("backend,ranks", [("gloo", 2), ("nccl", 2), ("gloo", 3)], ids=["gloo", "nccl", "gloo-3ranks"])
def test_bench_two_ranks_gather_the_single_rank_frame(pkg, tmp_path, backend, ranks):
    """bench.py's own step() with two ranks on one GPU -- samples accumulated straight in the gather's message
    (ptx_bind_shard_accumulation), ONE gather per step to the frame's owner, the owner ROTATING over the ranks (step k: rank k % 2),
    one ptx_unpack_shards launch that stores only to the host's frame, host frames in one shared-memory segment: EVERY frame of the
    job's store, whichever rank composed it, must be the single-rank frame bit for bit, and the JSON line must carry the
    strong-scaling metric with the weak one beside it, roofline.frac and the number of ranks the collective saw.
    The gloo variant starts WITHOUT a launcher: bench.py spawns its own ranks.
    With THREE ranks the world does not divide the 16 frames in flight: the rotating owner k % 3 against ring slot k % 16 gives
    lcm = 48 host frames, the shards are unequal (26 / 26 / 25 tiles), and F + warm-up + steps = 16 + 1 + 31 = 48 steps write every
    one of them once."""
    import json
    import time

    t0 = time.perf_counter()
    p, out = _run_bench_two_ranks(tmp_path, backend, launcher=(backend == "nccl"), ranks=ranks, extra=("--steps", "31") if ranks == 3 else ())
    print(f"bench.py with {ranks} {backend} ranks: {time.perf_counter() - t0:.1f} s wall")
    if p.returncode != 0 and backend == "nccl":
        # RCCL refuses two ranks on ONE device at communicator init ("Duplicate GPU detected", ncclInvalidUsage): that, and only
        # that, is a reason to skip -- any other failure of the RCCL branch is a failure of this test
        import re
        m = re.search(r"Duplicate GPU detected[^\n]*|ncclInvalidUsage[^\n]*|invalid usage[^\n]*", p.stderr + p.stdout)
        if m:
            pytest.skip("RCCL refuses two ranks on one device (runs wherever two GPUs exist): " + m.group(0)[:200])
    assert p.returncode == 0, p.stderr[-2000:]
    last = p.stdout.splitlines()[-1]  # the LAST stdout line parses on its own, under RCCL's stdout chatter too
    line = json.loads(last)
    assert len(last) < 4096
    assert line["n_gpus"] == ranks and line["n_ranks_seen"] == ranks and line["scaling"] == "strong" and line["weak"]["scaling"] == "weak" and line["value"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1  # the N > 1 line carries the CPU leg too
    assert 0 < line["roofline"]["frac"] < 1 and "rank k % N" in line["config"]["parallelism"]
    ref = _single_rank_frame(pkg)  # W, H = 328, 200: ragged, 328 is not a multiple of the 32-pixel tile
    got = np.load(out)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    frames = np.load(tmp_path / f"frames_{backend}.npy")
    assert frames.shape[0] == {2: 16, 3: 48}[ranks]  # lcm(ranks, 16 single-stream frames in flight); frame j composed by rank j % ranks
    assert line["config"]["frames_in_flight"] == 16 and "one stream" in line["config"]["parallelism"]
    for j in range(frames.shape[0]):
        assert (frames[j].view(np.uint32) == ref.view(np.uint32)).all(), f"frame {j} (owner: rank {j % ranks}) differs from the single-rank frame"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [("--root", "rank0"), ("--gather-unpack", "per-rank"), ("--shard-accumulation", "packed"),
                                     ("--root", "rank0", "--gather-unpack", "per-rank", "--shard-accumulation", "packed", "--gather-readback", "separate")])
def test_bench_two_ranks_older_gather_paths_give_the_same_frame(pkg, tmp_path, variant):
    """The step's round-1-5 forms stay selectable (rank 0 owns every frame; N unpack launches; row-major accumulation +
    ptx_pack_shard; separate read-back) and compose the same frame."""
    p, out = _run_bench_two_ranks(tmp_path, "gloo", extra=variant)
    assert p.returncode == 0, p.stderr[-2000:]
    ref = _single_rank_frame(pkg)
    assert (np.load(out).view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("collective", ["gather", "all_gather"])
def test_rccl_gather_branch_runs_with_one_rank(pkg, tmp_path, collective):
    """The RCCL branch of bench.py's step() on real hardware: a one-rank `nccl` process group (RCCL refuses two ranks on one
    device, and the GPU box has one), accumulation in the bound shard buffer -> dist.gather (grouped send / recv) on the renderer's
    torch stream -> one ptx_unpack_shards launch into the host's frame, frames in flight.  The gathered frame must be the plain frame bit
    for bit; the all_gather_into_tensor form of rounds 1-5 stays selectable and gives the same."""
    import json
    import subprocess

    out = tmp_path / "gathered_rccl1.npy"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()))
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--full", "--force-gather", "--dist-backend", "nccl", "--steps", "3", "--warmup", "1",
           "--repeats", "1", "--scene", "chess_like", "--detail", "0.05", "--width", "328", "--height", "200", "--spp", "4", "--depth", "6",
           "--in-flight", "3", "--cpu-seconds", "1", "--dump-image", str(out), "--collective", collective]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    last = p.stdout.splitlines()[-1]  # RCCL's own warnings go to fd 1 too: bench.py keeps them off the real stdout
    line = json.loads(last)
    assert len(last) < 4096 and line["cpu_baseline"]["value"] > 0
    assert line["n_gpus"] == 1 and line["n_ranks_seen"] == 1 and "gather" in line["config"]["parallelism"] and line["value"] > 0
    got = np.load(out)
    W, H = 328, 200
    scene = pkg.Scene("chess_like", 0.05)
    r = pkg.Renderer()
    r.upload(scene)
    r.resize(W, H)
    r.render_frames(scene.uniform(W, H, bounces=6), scene.lights, 0, 4)
    ref = r.readback()
    r.close()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
