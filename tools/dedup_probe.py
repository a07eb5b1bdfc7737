"""zk_dedup_frames_dev and zk_encode_dedup_dev timed beside the encode they spare: --mib MiB (1 GiB) of the bench's text
(oracle/zko.gen_chunks) resident in HBM, cut by zk_chunk_boundaries_dev at avg_size 4 KiB, 64 KiB and 2 MiB (min = avg / 4, max = 4 avg), in
two forms:
  as is                almost no duplicate chunks
  share s              every chunk i with (i * 2654435761 mod 2^32) / 2^32 < s, i >= 1, is replaced by a copy of the chunk before it in the
                       new list (so runs of copies occur), the list re-concatenated on the host and uploaded: the offsets are those of the
                       pieces, about s of the chunks and of the bytes are duplicates; the share of duplicate bytes is what the map reports
Per form, level 1, no checksums, ms = median of --repeats calls after a warm-up (host clock around a call that ends in a synchronise):
  map                  zk_dedup_frames_dev with all three outputs; from one profiled call the ms of its kernels
  dedup encode         zk_encode_dedup_dev
  list encode          zk_encode_frame_list_dev on the same offsets: the existing call, every frame encoded
and map / list encode (beside the 0.055 - 0.128 of the content-defined cuts, profiles/chunk_probe.txt), dedup encode / list encode, and per
avg_size the break-even share of duplicate bytes by linear interpolation between the two measured shares around it.
usage: python tools/dedup_probe.py [--out profiles/dedup_probe.txt] [--repeats 5] [--mib 1024] [--shares 0.125,0.25,0.5]"""
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
    ap.add_argument("--shares", default="0.125,0.25,0.5")
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
    say(f"# tools/dedup_probe.py on {eng.device_name}: {args.mib} MiB of the bench's text in HBM, level 1, no checksums; ms per call = median of {args.repeats} (min .. max)")
    host = np.frombuffer(zko.gen_chunks(n, 0), np.uint8)
    d_plain = torch.from_numpy(host.copy()).to(dev)
    shares = [float(s) for s in args.shares.split(",") if s]
    for avg in (4 << 10, 64 << 10, 2 << 20):
        off = eng.chunk_boundaries_dev(d_plain, n, avg_size=avg).cpu().numpy().view(np.uint64).astype(np.int64)
        count = len(off) - 1
        say(f"\n## avg_size {avg}: {count} chunks, mean {n / count:.0f} bytes")
        points = []
        for share in [0.0] + shares:
            if share == 0.0:
                d_src, new_off = d_plain, off
            else:
                take = np.arange(count)
                dup = ((np.arange(count, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32 < share
                dup[0] = False
                for i in np.nonzero(dup)[0]:
                    take[i] = take[i - 1]
                lens = (off[1:] - off[:-1])[take]
                new_off = np.concatenate([[0], np.cumsum(lens)])
                d_src = torch.from_numpy(np.concatenate([host[off[j]:off[j + 1]] for j in take])).to(dev)
            total = int(new_off[-1])
            d_off = torch.from_numpy(np.ascontiguousarray(new_off, dtype=np.int64)).to(dev)
            d_ref, d_ids, d_uniq, d_cs = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(4))
            cap = int(zk.lib.zk_compress_bound_list(total, count, 0))
            d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
            res = {}

            def the_map():
                res["nu"] = eng.dedup_frames_dev(d_src, d_off, count, d_ref, d_ids, d_uniq)

            def dedup_encode():
                res["dedup"] = eng.encode_dedup_dev(d_src, d_off, count, 1, False, d_dst, cap, d_ids, d_uniq, d_cs)

            def list_encode():
                res["list"] = eng.encode_frame_list_dev(d_src, d_off, count, 1, False, d_dst, cap)

            m = timed(the_map)
            zk.lib.zk_engine_set_profiling(eng._h, 1)
            the_map()
            kt = {k: v for k, v in eng.kernel_times().items() if k.startswith("zk_k_dedup")}
            zk.lib.zk_engine_set_profiling(eng._h, 0)
            de = timed(dedup_encode)
            le = timed(list_encode)
            nu = res["nu"]
            uniq = d_uniq[:nu].cpu().numpy().astype(np.int64)
            ubytes = int((new_off[uniq + 1] - new_off[uniq]).sum())
            dup_bytes = 1.0 - ubytes / total
            points.append((dup_bytes, de[0], le[0]))
            say(f"  share {share:.3f}: {count - nu} of {count} chunks are copies, {100 * dup_bytes:.2f} % of {total} bytes")
            say(f"    map           {m[0]:9.3f} ms  ({m[1]:.3f} .. {m[2]:.3f})   profiled: " + ", ".join(f"{k} {v:.3f}" for k, v in kt.items()))
            say(f"    dedup encode  {de[0]:9.3f} ms  ({de[1]:.3f} .. {de[2]:.3f})   {res['dedup'][1]} bytes written")
            say(f"    list encode   {le[0]:9.3f} ms  ({le[1]:.3f} .. {le[2]:.3f})   {res['list']} bytes written")
            say(f"    map / list encode = {m[0] / le[0]:.3f}   dedup encode / list encode = {de[0] / le[0]:.3f}")
            del d_dst, d_off
            if share != 0.0:
                del d_src
        even = "not reached up to the largest share measured"
        for (s0, d0, l0), (s1, d1, l1) in zip(points[:-1], points[1:]):
            if d0 - l0 > 0 >= d1 - l1:
                even = f"{100 * (s0 + (s1 - s0) * (d0 - l0) / ((d0 - l0) - (d1 - l1))):.1f} % of the bytes (between the shares measured at {100 * s0:.1f} % and {100 * s1:.1f} %)"
                break
        if points[0][1] <= points[0][2]:
            even = "0: the dedup encode is no slower without duplicates"
        say(f"  break-even share of duplicate bytes: {even}")
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
