"""zk_refine_entries_dev timed on the headline archive (2048 frames of 2 MiB, HBM-resident, level 1, checksummed), beside a decode of it:
  (a) the table as it is: 2048 entries of one frame (nothing to split: the walk + the size stages);
  (b) coarsened to 64 entries of 32 frames (64 lanes walk 32 frames each);
  (c) ONE entry without sizes: a stream nobody has a table for -- a single lane's chain of dependent loads, frame after frame.
Every refined table must equal (a)'s.  Three runs per case, each the median of five timed calls after one warm-up call; the source is
64 MiB of the generator's text tiled to 4 GiB on the device.  No threshold: nobody has measured any of this before.
usage: python tools/refine_probe.py [--out profiles/refine_probe.txt] [--gib 4]"""
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
    from oracle import zko
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = zk.Engine(0)
    say(f"# tools/refine_probe.py on {eng.device_name}")
    N, fs = args.gib << 30, 0x200000
    tile = torch.from_numpy(np.frombuffer(zko.gen_chunks(64 << 20, 0x8A11), np.uint8).copy()).to(dev)
    d_src = tile.repeat(N // tile.numel())
    del tile

    def u64(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64)).to(dev)

    nf = N // fs
    cap = int(zk.lib.zk_compress_bound(N, fs))
    d_comp = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
    d_cs = torch.zeros(nf, dtype=torch.int32, device=dev); d_ds = torch.zeros(nf, dtype=torch.int32, device=dev)
    n, csize = eng.encode_frames_dev(d_src, N, fs, 1, True, d_comp, cap, d_cs, d_ds)
    torch.cuda.synchronize()
    d_comp[csize:csize + 64] = 0
    c = np.zeros(n + 1, np.uint64); c[1:] = np.cumsum(d_cs.cpu().numpy().astype(np.uint64))
    d = np.zeros(n + 1, np.uint64); d[1:] = np.cumsum(d_ds.cpu().numpy().astype(np.uint64))
    say(f"archive: {n} frames of {fs} bytes, {csize} compressed bytes")

    d_co, d_do = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_eo = torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(fn):
        fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def case(name, cc, dd):
        m = len(cc) - 1
        d_c, d_d = u64(cc), (u64(dd) if dd is not None else None)
        d_st = torch.zeros(m, dtype=torch.int32, device=dev)

        def call():
            rc, got = eng.refine_entries_dev(d_comp, csize, d_c, d_d, m, d_co, d_do, d_eo, n, d_st)
            assert rc == 0 and got == n, (rc, got)
        ts = [timed(call) for _ in range(3)]
        assert np.array_equal(d_co.cpu().numpy().view(np.uint64), c) and np.array_equal(d_do.cpu().numpy().view(np.uint64), d), name
        say(f"{name}: zk_refine_entries_dev runs {', '.join(f'{t:.3f}' for t in ts)} ms (spread {max(ts) - min(ts):.3f})")

    case("(a) 2048 entries of one frame", c, d)
    case("(b) 64 entries of 32 frames", c[::32], d[::32])
    case("(c) one entry, no sizes", c[[0, n]], None)

    d_out = torch.empty(N + 64, dtype=torch.uint8, device=dev)
    d_c, d_d = u64(c), u64(d)

    def decode():
        assert eng.decode_frames_dev(d_comp, csize, d_c, d_d, 0, n, d_out, N, True) == 0
    ts = [timed(decode) for _ in range(3)]
    say(f"decode of the same archive (zk_decode_frames_dev, verified): runs {', '.join(f'{t:.3f}' for t in ts)} ms")
    assert torch.equal(d_out[:1 << 24], d_src[:1 << 24])
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
