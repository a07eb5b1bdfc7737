"""zk_dedup_against_dev and zk_encode_dedup_against_dev timed beside the in-call calls they extend: --mib MiB (1 GiB) of the
bench's text (oracle/zko.gen_chunks) resident in HBM, cut by zk_chunk_boundaries_dev at avg_size 4 KiB, 64 KiB and 2 MiB.
  generation 1         the whole list, appended to an empty archive with zk_encode_dedup_against_dev: the archive and its index
  generation 2         the same offsets; chunk i stays as it is -- the archive holds it -- when (i * 2654435761 mod 2^32) / 2^32 < s, and is
                       replaced by the bytes at its place in a second text otherwise (new content of the same length), for the stored shares
                       s = 0, 0.12, 0.5 and 1
Per share, level 1, no checksums, ms = median of --repeats calls after a warm-up (host clock around a call that ends in a synchronise; the
index is truncated back to generation 1 between the calls, outside the clock):
  against map          zk_dedup_against_dev with both outputs; from one profiled call its split into the in-call map (zk_k_dedup_*), the
                       lookup, the decode of the candidates (the decode kernels), the compare and the emit
  against encode       zk_encode_dedup_against_dev
  in-call map          zk_dedup_frames_dev on the same list          } the existing calls, the yardstick: nothing is known of the archive,
  in-call encode       zk_encode_dedup_dev on the same list          } every chunk is encoded
and per avg_size the stored share from which the new call is the faster one, by linear interpolation between the measured shares around it.
usage: python tools/dedup_against_probe.py [--out profiles/dedup_against_probe.txt] [--repeats 5] [--mib 1024] [--shares 0,0.12,0.5,1]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECODE = ("zk_k_walk(count)", "zk_k_scan", "zk_k_walk(fill)", "zk_k_huf", "zk_k_fse", "zk_k_exec", "zk_k_xxh64", "zk_k_status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--shares", default="0,0.12,0.5,1")
    ap.add_argument("--avgs", default="4096,65536,2097152")
    args = ap.parse_args()
    import torch
    import zeekstd_amd as zk
    from oracle import zko
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, after=None):
        fn()
        if after:
            after()
        ts = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            if after:
                after()
        return statistics.median(ts), min(ts), max(ts)

    eng = zk.Engine(0)
    n = args.mib << 20
    say(f"# tools/dedup_against_probe.py on {eng.device_name}: {args.mib} MiB of the bench's text in HBM, level 1, no checksums; ms per call = median of {args.repeats} (min .. max)")
    d_plain = torch.from_numpy(np.frombuffer(zko.gen_chunks(n, 0), np.uint8).copy()).to(dev)
    d_other = torch.from_numpy(np.frombuffer(zko.gen_chunks(n, 1), np.uint8).copy()).to(dev)
    shares = [float(s) for s in args.shares.split(",") if s]
    for avg in [int(a) for a in args.avgs.split(",") if a]:
        d_off = eng.chunk_boundaries_dev(d_plain, n, avg_size=avg).clone()
        off = d_off.cpu().numpy().view(np.uint64).astype(np.int64)
        count = len(off) - 1
        cap = int(zk.lib.zk_compress_bound_list(n, count, 0))
        d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        d_ids, d_fresh, d_cs, d_ds, d_ref = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(5))
        # generation 1: the archive
        index = zk.DedupIndex(eng)
        empty = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, wr = eng.encode_dedup_against_dev(index, d_dst, 0, empty, empty, 0, d_plain, d_off, count, 1, False, d_dst, cap, d_ids, d_fresh, d_cs, d_ds)
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        d_comp = torch.zeros(wr + 64, dtype=torch.uint8, device=dev)
        d_comp[:wr] = d_dst[:wr]
        to_off = lambda t: torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(t[:m].to(torch.int64) & 0xFFFFFFFF, 0)])
        d_c_off, d_d_off = to_off(d_cs), to_off(d_ds)
        say(f"\n## avg_size {avg}: {count} chunks, mean {n / count:.0f} bytes; generation 1 (first call, cold): {m} frames, {wr} bytes, {first_ms:.1f} ms")
        lens = torch.from_numpy(off[1:] - off[:-1]).to(dev)
        points = []
        for share in shares:
            stored = ((np.arange(count, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32 < share
            keep = torch.repeat_interleave(torch.from_numpy(stored).to(dev), lens)
            d_src = torch.where(keep, d_plain, d_other)
            del keep
            kept_bytes = int((off[1:] - off[:-1])[stored].sum())
            res = {}
            back = lambda: index.truncate(m)

            def against_map():
                res["nf"] = eng.dedup_against_dev(index, d_comp, wr, d_c_off, d_d_off, m, d_src, d_off, count, d_ids, d_fresh)

            def against_encode():
                res["against"] = eng.encode_dedup_against_dev(index, d_comp, wr, d_c_off, d_d_off, m, d_src, d_off, count, 1, False, d_dst, cap, d_ids, d_fresh, d_cs, d_ds)

            def in_call_map():
                res["nu"] = eng.dedup_frames_dev(d_src, d_off, count, d_ref, d_ids, d_fresh)

            def in_call_encode():
                res["in_call"] = eng.encode_dedup_dev(d_src, d_off, count, 1, False, d_dst, cap, d_ids, d_fresh, d_cs)

            am = timed(against_map)
            zk.lib.zk_engine_set_profiling(eng._h, 1)
            against_map()
            kt = eng.kernel_times()
            zk.lib.zk_engine_set_profiling(eng._h, 0)
            split = {"in-call map": sum(v for k, v in kt.items() if k.startswith("zk_k_dedup")), "lookup": kt.get("zk_k_dxi_lookup", 0.0),
                     "decode": sum(kt.get(k, 0.0) for k in DECODE), "compare": kt.get("zk_k_dxi_compare", 0.0), "emit": kt.get("zk_k_dxi_emit", 0.0)}
            ae = timed(against_encode, back)
            im = timed(in_call_map)
            ie = timed(in_call_encode)
            points.append((share, ae[0], ie[0]))
            say(f"  stored share {share:.2f}: {int(stored.sum())} of {count} chunks, {100 * kept_bytes / n:.2f} % of the bytes; {res['nf']} fresh")
            say(f"    against map      {am[0]:9.3f} ms  ({am[1]:.3f} .. {am[2]:.3f})   profiled (kernels only): " + ", ".join(f"{k} {v:.3f}" for k, v in split.items()))
            say(f"    against encode   {ae[0]:9.3f} ms  ({ae[1]:.3f} .. {ae[2]:.3f})   {res['against'][1]} bytes written, {res['against'][0]} frames")
            say(f"    in-call map      {im[0]:9.3f} ms  ({im[1]:.3f} .. {im[2]:.3f})")
            say(f"    in-call encode   {ie[0]:9.3f} ms  ({ie[1]:.3f} .. {ie[2]:.3f})   {res['in_call'][1]} bytes written, {res['in_call'][0]} frames")
            say(f"    against map / in-call map = {am[0] / im[0]:.2f}   against encode / in-call encode = {ae[0] / ie[0]:.3f}")
            del d_src
        even = "not reached up to the largest share measured"
        for (s0, a0, i0), (s1, a1, i1) in zip(points[:-1], points[1:]):
            if a0 - i0 > 0 >= a1 - i1:
                even = f"{100 * (s0 + (s1 - s0) * (a0 - i0) / ((a0 - i0) - (a1 - i1))):.1f} % of the chunks (between the shares measured at {100 * s0:.0f} % and {100 * s1:.0f} %)"
                break
        if points and points[0][1] <= points[0][2]:
            even = f"{100 * points[0][0]:.0f} %: the new call is no slower at the smallest share measured"
        say(f"  stored share from which zk_encode_dedup_against_dev is the faster call: {even}")
        index.close()
        del d_dst, d_comp
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
