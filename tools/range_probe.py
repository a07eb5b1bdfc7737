"""Batched byte-range reads, two ways of getting the same bytes into one packed device buffer, timed alternately in one process:
  (a) what a caller does without zk_read_ranges_dev: np.searchsorted on the host, the frame list made unique, uploads,
      decode_frame_list_dev of whole frames, torch slicing + cat to pack the wanted bytes;
  (b) Engine.read_ranges_dev.
Shapes (HBM-resident, checksums verified): (i) 65 536 x 64 KiB frames, 1 024 reads of bench.seek_protocol; (ii) 2 048 x 2 MiB frames,
1 024 reads of 4 KiB; (iii) the same archive, 64 reads of 1 MiB at odd offsets; (iv) 1 024 reads that fall into 32 frames.
Three runs per shape and way, each the median of seven timed calls after two warm-up calls; the source is 64 MiB of the generator's
text tiled to 4 GiB on the device.  usage: python tools/range_probe.py [--out profiles/r08_read_ranges.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=int, default=4)
    args = ap.parse_args()
    import torch
    import zeekstd_amd as zk
    import bench
    from oracle import zko
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = zk.Engine(0)
    say(f"# tools/range_probe.py on {eng.device_name}")
    N = args.gib << 30
    tile = torch.from_numpy(np.frombuffer(zko.gen_chunks(64 << 20, 0x8A11), np.uint8).copy()).to(dev)
    d_src = tile.repeat(N // tile.numel())
    del tile

    def u64(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64)).to(dev)

    def archive(fs):
        nf = N // fs
        cap = int(zk.lib.zk_compress_bound(N, fs))
        d_comp = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        d_cs = torch.zeros(nf, dtype=torch.int32, device=dev); d_ds = torch.zeros(nf, dtype=torch.int32, device=dev)
        n, csize = eng.encode_frames_dev(d_src, N, fs, 1, True, d_comp, cap, d_cs, d_ds)
        torch.cuda.synchronize()
        comp = d_comp[:csize + 64].clone(); comp[csize:] = 0
        del d_comp
        torch.cuda.empty_cache()
        c = np.zeros(n + 1, np.uint64); c[1:] = np.cumsum(d_cs.cpu().numpy().astype(np.uint64))
        d = np.zeros(n + 1, np.uint64); d[1:] = np.cumsum(d_ds.cpu().numpy().astype(np.uint64))
        return dict(comp=comp, csize=csize, c=c, d=d, n=n, d_c=u64(c), d_d=u64(d))

    def way_a(A, offs, lens):
        d = A["d"]
        first = np.searchsorted(d, offs, "right") - 1
        last = np.searchsorted(d, offs + lens - np.uint64(1), "right") - 1
        ids = np.unique(np.concatenate([np.arange(f, l + 1) for f, l in zip(first, last)])).astype(np.uint32)
        sizes = (d[ids.astype(np.int64) + 1] - d[ids.astype(np.int64)]).astype(np.uint64)
        oo = np.zeros(len(ids) + 1, np.uint64); oo[1:] = np.cumsum(sizes)
        buf = torch.empty(int(oo[-1]) + 64, dtype=torch.uint8, device=dev)
        d_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
        rc = eng.decode_frame_list_dev(A["comp"], A["csize"], A["d_c"], A["d_d"], d_ids, u64(oo), len(ids), buf, int(oo[-1]), True)
        assert rc == 0
        start = oo[np.searchsorted(ids, first)].astype(np.int64) + (offs - d[first]).astype(np.int64)      # touched frames are adjacent in buf
        out = torch.cat([buf[s:s + n] for s, n in zip(start.tolist(), lens.astype(np.int64).tolist())])
        torch.cuda.synchronize()
        return out

    def way_b(A, offs, lens, d_o=None, d_l=None):
        out = torch.empty(int(lens.sum()) + 64, dtype=torch.uint8, device=dev)
        rc = eng.read_ranges_dev(A["comp"], A["csize"], A["d_c"], A["d_d"], A["n"], u64(offs), u64(lens), None, len(offs), out, int(lens.sum()), True)
        assert rc == 0
        return out[:int(lens.sum())]

    def timed(fn, *a):
        for _ in range(2):
            fn(*a)
        ts = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(*a)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def shape(name, A, offs, lens):
        offs, lens = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
        a, b = way_a(A, offs, lens), way_b(A, offs, lens)
        assert torch.equal(a, b), name
        want = torch.cat([d_src[int(o):int(o + n)] for o, n in zip(offs[:64], lens[:64])])
        assert torch.equal(b[:want.numel()], want), name
        del a, b, want
        ta, tb = [], []
        for _ in range(3):
            ta.append(timed(way_a, A, offs, lens))
            tb.append(timed(way_b, A, offs, lens))
        eng.set_profiling(True)
        way_b(A, offs, lens); way_b(A, offs, lens)
        kt = eng.kernel_times()
        eng.set_profiling(False)
        say(f"{name}: {len(offs)} reads, {int(lens.sum())} bytes wanted, {eng.ranges_frames_decoded()} frames touched")
        say(f"  (a) searchsorted + decode_frame_list_dev + cat: runs {', '.join(f'{t:.3f}' for t in ta)} ms (spread {max(ta) - min(ta):.3f})")
        say(f"  (b) read_ranges_dev:                            runs {', '.join(f'{t:.3f}' for t in tb)} ms   median (b) / median (a) = {np.median(tb) / np.median(ta):.3f}")
        say("  (b) per kernel, profiling on (kernels serialised), ms: " + ", ".join(f"{k} {v:.3f}" for k, v in kt.items()))
        return kt

    rng = np.random.default_rng(0x8A12)
    A64 = archive(65536)
    offs, lens = bench.seek_protocol(1024, N)
    lens = np.minimum(lens.astype(np.uint64), np.uint64(N) - offs)
    shape("(i) 65536 x 64 KiB frames, seek_protocol", A64, offs, lens)
    del A64
    torch.cuda.empty_cache()
    A2 = archive(0x200000)
    shape("(ii) 2048 x 2 MiB frames, 1024 x 4 KiB", A2, rng.integers(0, N - 4096, 1024).astype(np.uint64), np.full(1024, 4096, np.uint64))
    o3 = (rng.integers(0, N - (1 << 20), 64) | 1).astype(np.uint64)
    kt = shape("(iii) 2048 x 2 MiB frames, 64 x 1 MiB at odd offsets", A2, o3, np.full(64, 1 << 20, np.uint64))
    if kt.get("zk_k_range_gather"):
        say(f"  zk_k_range_gather: {64 * (1 << 20) / (kt['zk_k_range_gather'] * 1e-3) / 1e9:.1f} GB/s copied (read + write: twice that in traffic)")
    f32 = rng.choice(A2["n"], 32, replace=False).astype(np.uint64)
    o4 = f32[rng.integers(0, 32, 1024)] * np.uint64(0x200000) + rng.integers(0, 0x200000 - 4096, 1024).astype(np.uint64)
    shape("(iv) 1024 x 4 KiB in 32 frames of 2 MiB", A2, o4, np.full(1024, 4096, np.uint64))

    # peak device memory of both ways on (ii): what the device reports as used, against the state before the first call of a fresh engine
    offs2, lens2 = rng.integers(0, N - 4096, 1024).astype(np.uint64), np.full(1024, 4096, np.uint64)
    for name, fn in (("(a)", way_a), ("(b)", way_b)):
        eng.close()
        eng = zk.Engine(0)
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info(dev)[0]
        fn(A2, offs2, lens2)
        free1 = torch.cuda.mem_get_info(dev)[0]          # (torch's cache and the engine's scratch both keep what they took)
        say(f"(ii) device memory taken by {name}: {(free0 - free1) / 2**20:.0f} MiB")
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
