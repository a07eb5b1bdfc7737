"""zk_compact_archive_dev and zk_dedup_index_compact_dev timed beside the copy they cannot beat: --mib MiB (1 GiB) of the
bench's text (oracle/zko.gen_chunks) resident in HBM, cut by zk_chunk_boundaries_dev at avg_size 4 KiB, 64 KiB and 2 MiB and appended to an
empty archive with zk_encode_dedup_against_dev at level 1 (what DedupStore.append calls): the archive and its index.  Per avg_size the
archive loses, in turn, every other frame, a random 10 % of its frames, its older half and its newer half; each out of place (into a second
buffer) and in place (on a copy that is restored between the calls, outside the clock).
Per removal, ms = median of --repeats calls after a warm-up (host clock around a call that ends in a synchronise, as in the other probes):
  whole call           zk_compact_archive_dev with remap and both offset arrays written
  move / bookkeeping   from one profiled call: zk_k_cmp_move (in place: every step, the staged steps' copies included) and zk_k_cmp_emit (the
                       flags, the three scans, the emit and, in place, the steps' gaps)
  copy                 a plain device-to-device copy of `written` bytes in the same run: the yardstick.  A compaction cannot beat the copy
                       of the bytes it keeps; a staged step moves its bytes twice
  index                zk_dedup_index_compact_dev against the alternative it replaces, zk_dedup_index_add_archive_dev into an empty index
                       over the compacted archive (which decodes every kept frame)
usage: python tools/compact_probe.py [--out profiles/compact_probe.txt] [--repeats 5] [--mib 1024]"""
import argparse
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

    def profiled(fn, after=None):
        zk.lib.zk_engine_set_profiling(eng._h, 1)
        fn()
        kt = eng.kernel_times()
        zk.lib.zk_engine_set_profiling(eng._h, 0)
        if after:
            after()
        return kt.get("zk_k_cmp_move", 0.0), kt.get("zk_k_cmp_emit", 0.0)

    eng = zk.Engine(0)
    n = args.mib << 20
    say(f"# tools/compact_probe.py on {eng.device_name}: {args.mib} MiB of the bench's text in HBM, stored at level 1 without checksums; ms per call = median of {args.repeats} (min .. max)")
    d_plain = torch.from_numpy(np.frombuffer(zko.gen_chunks(n, 0), np.uint8).copy()).to(dev)
    for avg in [int(a) for a in args.avgs.split(",") if a]:
        d_off = eng.chunk_boundaries_dev(d_plain, n, avg_size=avg).clone()
        count = d_off.numel() - 1
        cap = int(zk.lib.zk_compress_bound_list(n, count, 0))
        d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        d_ids, d_fresh, d_cs, d_ds = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(4))
        index = zk.DedupIndex(eng)
        empty = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        m, wr = eng.encode_dedup_against_dev(index, d_dst, 0, empty, empty, 0, d_plain, d_off, count, 1, False, d_dst, cap, d_ids, d_fresh, d_cs, d_ds)
        d_comp = torch.zeros(wr + 64, dtype=torch.uint8, device=dev)
        d_comp[:wr] = d_dst[:wr]
        del d_dst
        to_off = lambda t: torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(t[:m].to(torch.int64) & 0xFFFFFFFF, 0)])
        d_c_off, d_d_off = to_off(d_cs), to_off(d_ds)
        c_sizes = (d_cs[:m].cpu().numpy().view(np.uint32)).astype(np.int64)
        keys, lens = index.export()
        say(f"\n## avg_size {avg}: {count} chunks, {m} frames stored, {wr} bytes ({wr / m:.0f} per frame)")
        d_work, d_out = torch.empty_like(d_comp), torch.empty_like(d_comp)
        d_c_out, d_d_out = torch.empty_like(d_c_off), torch.empty_like(d_d_off)
        d_remap = torch.zeros(m, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(7)
        removals = {"every other frame": (np.arange(m) & 1) == 0, "a random 10 %": rng.random(m) >= 0.10, "the older half": np.arange(m) >= m // 2,
                    "the newer half": np.arange(m) < m // 2}
        for name, live in removals.items():
            d_live = torch.from_numpy(live.astype(np.uint8)).to(dev)
            kept_bytes = int(c_sizes[live].sum())
            res = {}
            restore = lambda: d_work.copy_(d_comp)

            def out_of_place():
                res["out"] = eng.compact_archive_dev(d_comp, wr, d_c_off, d_d_off, m, d_live, d_out, wr, d_c_out, d_d_out, d_remap)

            def in_place():
                res["in"] = eng.compact_archive_dev(d_work, wr, d_c_off, d_d_off, m, d_live, d_work, wr, d_c_out, d_d_out, d_remap)

            def copy():
                d_out[:kept_bytes].copy_(d_comp[:kept_bytes])

            restore()
            torch.cuda.synchronize()
            o, i, c = timed(out_of_place), timed(in_place, restore), timed(copy)
            po, pi = profiled(out_of_place), profiled(in_place, restore)
            assert res["out"] == res["in"] == (int(live.sum()), kept_bytes)
            in_place()
            torch.cuda.synchronize()
            assert torch.equal(d_work[:kept_bytes], d_out[:kept_bytes])
            say(f"  removed: {name}: {int(live.sum())} of {m} frames and {kept_bytes} bytes ({100 * kept_bytes / wr:.1f} %) kept")
            say(f"    copy of written   {c[0]:9.3f} ms  ({c[1]:.3f} .. {c[2]:.3f})   {kept_bytes / c[0] / 1e6:.0f} GB/s")
            say(f"    out of place      {o[0]:9.3f} ms  ({o[1]:.3f} .. {o[2]:.3f})   profiled: move {po[0]:.3f}, bookkeeping {po[1]:.3f}; move / copy = {po[0] / c[0]:.2f}")
            say(f"    in place          {i[0]:9.3f} ms  ({i[1]:.3f} .. {i[2]:.3f})   profiled: move {pi[0]:.3f}, bookkeeping {pi[1]:.3f}; move / copy = {pi[0] / c[0]:.2f}")
            # the index: compacted, against decoded again from the compacted archive
            kept = np.nonzero(live)[0]
            made = {}

            def fresh_full():
                if "x" in made:
                    made["x"].close()
                made["x"] = zk.DedupIndex(eng)
                made["x"].add(keys, lens)

            def fresh_empty():
                if "y" in made:
                    made["y"].close()
                made["y"] = zk.DedupIndex(eng)

            fresh_full()
            fresh_empty()
            xc = timed(lambda: made["x"].compact_dev(d_remap, m), fresh_full)
            xa = timed(lambda: made["y"].add_archive_dev(d_out, kept_bytes, d_c_out, d_d_out, len(kept)), fresh_empty)
            made["x"].compact_dev(d_remap, m)
            k2, l2 = made["x"].export()
            assert (k2 == keys[kept]).all() and (l2 == lens[kept]).all()
            say(f"    index compact     {xc[0]:9.3f} ms  ({xc[1]:.3f} .. {xc[2]:.3f})   against zk_dedup_index_add_archive_dev over the compacted archive: {xa[0]:.3f} ms ({xa[1]:.3f} .. {xa[2]:.3f})")
            made["x"].close()
            made["y"].close()
        index.close()
        del d_comp, d_work, d_out
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
