"""The N>1 path on CPU: world_size-2 and world_size-8 gloo processes run the same gather code the GPUs run over RCCL
(zeekstd_amd/parallel.py): shard ranges, size exchange, point-to-point payload gather, seek-entry gather,
seek table appended on the root.  The per-rank encoder here is the CPU oracle (test infrastructure) --
the collective logic is what is under test; the GPU encoder is covered by tests/test_gpu_encode.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import zko

FS = 1000


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, n_total, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from zeekstd_amd import parallel
    data = zko.gen_text(n_total, 99)
    nframes = -(-n_total // FS)
    lo, hi = parallel.shard_range(nframes, rank, world)
    frames, payload = [], bytearray()
    for f in range(lo, hi):
        chunk = data[f * FS:(f + 1) * FS]
        fr = zko.frame_encode(chunk, 1, True)
        payload += fr
        frames.append((len(fr), len(chunk)))
    t = torch.frombuffer(bytearray(payload), dtype=torch.uint8) if payload else torch.zeros(0, dtype=torch.uint8)
    cs = torch.tensor([f[0] for f in frames], dtype=torch.int32)
    ds = torch.tensor([f[1] for f in frames], dtype=torch.int32)
    out, table = parallel.gather_seekable(t, cs, ds, root=0)
    if rank == 0:
        q.put((bytes(out.numpy()), table.to_bytes()))
    else:
        assert out is None and table is None
    dist.barrier()
    dist.destroy_process_group()


# world 8 = configs[4]'s shape (BASELINE.json: frames sharded over the 8 GPUs of a node): more ranks than frames, ranks with nothing,
# the root's slice at the front -- the rank arithmetic the 8-GPU run depends on and no 1-GPU box can exercise
@pytest.mark.parametrize("n_total,world", [(7321, 2), (1000, 2), (999, 2), (123456, 2), (123456, 8), (2500, 8), (999, 8)])
def test_gather_seekable_world2(n_total, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_total, q)) for r in range(world)]
    for p in procs:
        p.start()
    stream, tbytes = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    # the gathered stream is a valid seekable archive: table at the tail, frames in global order
    import zeekstd_amd as zk
    data = zko.gen_text(n_total, 99)
    assert stream.endswith(tbytes)
    st = zk.SeekTable.from_seekable(stream)
    assert st.num_frames() == -(-n_total // FS) and st.size_decomp() == n_total
    assert st.size_comp() + len(tbytes) == len(stream)
    out = bytearray()
    for i in range(st.num_frames()):
        fr = stream[st.frame_start_comp(i):st.frame_end_comp(i)]
        dec, used = zko.frame_decode(fr, st.frame_size_decomp(i), True)
        assert used == len(fr)
        out += dec
    assert bytes(out) == data


def test_shard_range_partitions_everything():
    from zeekstd_amd import parallel
    for n in (0, 1, 7, 8, 9, 2048, 16384, 16385):
        for w in (1, 2, 3, 8):
            got = [parallel.shard_range(n, r, w) for r in range(w)]
            assert got[0][0] == 0 and got[-1][1] == n
            assert all(got[i][1] == got[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in got]
            assert max(sizes) - min(sizes) <= 1


# ---------------------------------------------------------------- encode_sharded itself, on CPU
class FakeEngine:
    """Stands in for zeekstd_amd.Engine in the gloo tests: encode_frames_dev with the engine's signature, the frames made by
    the CPU twin of the GPU encoder (test infrastructure).  What is under test is parallel.encode_sharded -- the function the
    GPU ranks call -- not the codec."""

    def encode_frames_dev(self, d_src, n, frame_size, level, checksum, d_comp, cap, d_cs, d_ds, stream=None):
        data = bytes(d_src[:n].numpy())
        nf = max(1, -(-n // frame_size))
        pos = 0
        for f in range(nf):
            chunk = data[f * frame_size:(f + 1) * frame_size]
            fr = zko.frame_encode(chunk, level, checksum)
            assert pos + len(fr) <= cap
            d_comp[pos:pos + len(fr)] = torch.frombuffer(bytearray(fr), dtype=torch.uint8)
            d_cs[f] = len(fr); d_ds[f] = len(chunk)
            pos += len(fr)
        return nf, pos


def _worker_sharded(rank, world, port, n_total, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from zeekstd_amd import parallel
    data = zko.gen_text(n_total, 77)
    nframes = -(-n_total // FS)
    lo, hi = parallel.shard_range(nframes, rank, world)
    shard = data[lo * FS:min(hi * FS, n_total)]
    d_src = torch.frombuffer(bytearray(shard), dtype=torch.uint8) if shard else torch.zeros(0, dtype=torch.uint8)
    if lo == hi:                                   # a rank without frames contributes nothing
        out, table = parallel.gather_seekable(torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.int32),
                                              torch.zeros(0, dtype=torch.int32), root=0)
    else:
        out, table = parallel.encode_sharded(FakeEngine(), d_src, FS, 1, True, root=0)
    if rank == 0:
        q.put((bytes(out.numpy()), table.num_frames()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_total,world", [(5 * FS + 17, 2), (FS, 2), (64 * FS, 2), (64 * FS + 5, 8), (3 * FS, 8)])
def test_encode_sharded_world2(n_total, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_sharded, args=(r, world, port, n_total, q)) for r in range(world)]
    for p in procs:
        p.start()
    stream, nfr = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    import zeekstd_amd as zk
    data = zko.gen_text(n_total, 77)
    st = zk.SeekTable.from_seekable(stream)
    assert st.num_frames() == nfr == -(-n_total // FS) and st.size_decomp() == n_total
    out = bytearray()
    for i in range(st.num_frames()):
        fr = stream[st.frame_start_comp(i):st.frame_end_comp(i)]
        out += zko.frame_decode(fr, st.frame_size_decomp(i), True)[0]
    assert bytes(out) == data


@pytest.mark.parametrize("world", [2, 8])
def test_bench_dry_run_world2(world):
    """bench.py's N > 1 control flow (env parsing, process group, shard + gather leg, the JSON line) under gloo, no GPU -- as the
    driver launches it for N = 2 and for the node's 8."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = _free_port()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), "bench.py", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--dry-run", "--full"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["steps"] == 2 and d["warmup"] == 1 and d["dry_run"] is True and d["scaling"] == "weak"
    g = d["rccl_gather"]                                     # the exchange leg's result is IN the line: frames, bytes, ms
    assert g["frames_on_root"] == world * d["config"]["frames_per_gpu"] and g["ms"] > 0
    assert g["stream_bytes_on_root"] == world * 4 * (1000 + 9) + world * 4 * 8 + 17


def _worker_too_small(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import datetime
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from zeekstd_amd import parallel
    payload = torch.full((5000 + 100 * rank,), rank, dtype=torch.uint8)
    cs = torch.tensor([payload.numel()], dtype=torch.int32)
    ds = torch.tensor([20000], dtype=torch.int32)
    verdicts = []
    # the root's room: too small by one byte, then exactly enough (5000 + 5100 bytes of payload + 8 * 2 + 17 of table)
    for cap in (10132, 10133):
        try:
            out, table = parallel.gather_seekable(payload, cs, ds, root=0, out_cap=cap if rank == 0 else None)
            verdicts.append("ok" if (out is not None) == (rank == 0) else "bad")
            if rank == 0:
                assert out.numel() == 10133 and table.num_frames() == 2
        except parallel.GatherTooSmall:
            verdicts.append("too_small")
    q.put((rank, verdicts))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_failure_is_agreed_on_by_every_rank():
    """VERDICT r2 #14 / ADVICE: a root whose destination is too small used to return alone while its peers went on to send
    (a hang until the communicator timed out).  The root's capacity now travels with the sizes: every rank raises the same
    error before a send or receive is posted, and the next collective on the same group works."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_too_small, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got == {0: ["too_small", "ok"], 1: ["too_small", "ok"]}
