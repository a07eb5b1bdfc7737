"""zk_chunk_boundaries_dev timed beside the encode it feeds: 1 GiB of the bench's text (oracle/zko.gen_chunks) resident in HBM,
avg_size 2 MiB, 64 KiB and 4 KiB with the default min = avg / 4 and max = 4 avg.  Per setting:
  boundaries           the whole zk_chunk_boundaries_dev call into an array of n / min + 1 entries (one pass), median of --repeats calls after a
                       warm-up (host clock around a call that ends in a synchronise); from one profiled call the ms of zk_k_cdc_mark and of
                       zk_k_cdc_select, added up over the slices
  list encode          zk_encode_frame_list_dev, level 1, no checksums, on those offsets: ms and ratio
  uniform encode       zk_encode_frames_dev at frame_size = min + avg, the mean the rule aims at: ms and ratio
and boundaries / list encode, the quotient DESIGN.md's decision about a parallel selection goes by (at 64 KiB: build it above 0.25).
usage: python tools/chunk_probe.py [--out profiles/chunk_probe.txt] [--repeats 5] [--mib 1024]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1024)
    args = ap.parse_args()
    import torch
    import zeekstd_amd as zk
    from oracle import zko
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    eng = zk.Engine(0)
    n = args.mib << 20
    say(f"# tools/chunk_probe.py on {eng.device_name}: {args.mib} MiB of the bench's text in HBM; ms per call = median of {args.repeats} (min .. max)")
    d_src = torch.from_numpy(np.frombuffer(zko.gen_chunks(n, 0), np.uint8).copy()).to(dev)
    for avg in (2 << 20, 64 << 10, 4 << 10):
        mn, mx = avg // 4, 4 * avg
        cap = n // mn + 1
        d_off = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        par = zk._lib.ChunkParams(mn, avg, mx, 0)
        count = C.c_uint32()

        def boundaries():
            rc = zk.lib.zk_chunk_boundaries_dev(eng._h, d_src.data_ptr(), n, C.byref(par), d_off.data_ptr(), cap, C.byref(count), None)
            assert rc == 0, rc

        b = timed(boundaries)
        frames = count.value
        eng.set_profiling(True)
        boundaries()
        kt = eng.kernel_times()
        eng.set_profiling(False)
        fs = mn + avg
        dst_cap = max(int(zk.lib.zk_compress_bound_list(n, frames, 0)), int(zk.lib.zk_compress_bound(n, fs)))
        d_dst = torch.empty(dst_cap + 64, dtype=torch.uint8, device=dev)
        written = {}

        def list_encode():
            written["list"] = eng.encode_frame_list_dev(d_src, d_off, frames, 1, False, d_dst, dst_cap)

        def uniform_encode():
            written["uniform"] = eng.encode_frames_dev(d_src, n, fs, 1, False, d_dst, dst_cap)[1]

        le = timed(list_encode)
        ue = timed(uniform_encode)
        say(f"\n## avg_size {avg} (min {mn}, max {mx}): {frames} frames, mean {n / frames:.0f} bytes")
        say(f"  boundaries      {b[0]:9.3f} ms  ({b[1]:.3f} .. {b[2]:.3f})  {n / (1 << 30) / (b[0] / 1e3):8.2f} GiB/s;"
            f"  profiled: zk_k_cdc_mark {kt.get('zk_k_cdc_mark', 0):.3f} ms, zk_k_cdc_select {kt.get('zk_k_cdc_select', 0):.3f} ms")
        say(f"  list encode     {le[0]:9.3f} ms  ({le[1]:.3f} .. {le[2]:.3f})  {n / (1 << 30) / (le[0] / 1e3):8.2f} GiB/s  ratio {n / written['list']:.3f}")
        say(f"  uniform encode  {ue[0]:9.3f} ms  ({ue[1]:.3f} .. {ue[2]:.3f})  {n / (1 << 30) / (ue[0] / 1e3):8.2f} GiB/s  ratio {n / written['uniform']:.3f}"
            f"  (frame_size {fs})")
        say(f"  boundaries / list encode = {b[0] / le[0]:.3f}")
        del d_dst, d_off
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
