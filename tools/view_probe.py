"""zk_read_view_ranges_dev timed beside the routes it replaces: --mib MiB (1 GiB) of the bench's text (oracle/zko.gen_chunks)
resident in HBM, cut by zk_chunk_boundaries_dev at avg_size 4 KiB, 64 KiB and 2 MiB and stored with zk_encode_dedup_against_dev at level 1 (what
DedupStore.append calls): snapshot A.  Snapshot B has A's cuts, every other chunk A's and the others the same text from elsewhere: half its chunks repeat frames the
archive holds (but none of its own).  Snapshot C is every even chunk of A twice in a row: half its chunks repeat chunks of its own.  Per avg_size, ms = median of --repeats calls after a warm-up (host clock around a call that ends in a synchronise):
  restore        one range over the whole view, against zk_decode_frame_list_dev with d_ids = ids (the parent's route: it decodes a frame once
                 per occurrence), for A, B and C; and, from one profiled call, the plan kernels (zk_k_view_plan + zk_k_view_mark), the gather
                 and the decode kernels apart, the gather beside a plain device copy of the bytes delivered
  random reads   1 024 and 65 536 random 4 KiB ranges and 16 ranges of 16 MiB through B's view, against zk_read_ranges_dev with the same shapes
                 on the archive's own stream; plan / gather / decode apart as above
usage: python tools/view_probe.py [--out profiles/view_probe.txt] [--repeats 5] [--mib 1024]"""
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

    def profiled(fn):
        eng.set_profiling(True)
        fn()
        kt = eng.kernel_times()
        eng.set_profiling(False)
        return kt

    def parts(kt, view):
        plan = kt.get("zk_k_view_plan", 0.0) + kt.get("zk_k_view_mark", 0.0) if view else kt.get("zk_k_range_plan", 0.0) + kt.get("zk_k_range_pieces", 0.0)
        gather = kt.get("zk_k_view_gather" if view else "zk_k_range_gather", 0.0)
        return plan, gather, sum(kt.get(k, 0.0) for k in DECODE)

    fmt = lambda t: f"{t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f})"
    u64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64)).view(np.int64).copy()).to(dev)

    eng = zk.Engine(0)
    eng.set_kernel_choice(range_pass_mib=4096)               # one pass: the per-kernel times of a call are those of its last pass
    n = args.mib << 20
    say(f"# tools/view_probe.py on {eng.device_name}: {args.mib} MiB of the bench's text in HBM, stored at level 1 without checksums; ms per call = median of {args.repeats} (min .. max)")
    d_a = torch.from_numpy(np.frombuffer(zko.gen_chunks(n, 0), np.uint8).copy()).to(dev)
    d_new = torch.roll(d_a, 12345677)                        # the same text somewhere else: no chunk of it is a chunk of A
    d_out = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    d_copy = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    for avg in [int(a) for a in args.avgs.split(",") if a]:
        d_off = eng.chunk_boundaries_dev(d_a, n, avg_size=avg).clone()
        off = d_off.cpu().numpy().view(np.uint64)
        count = len(off) - 1
        # snapshot B: A's cuts, the odd chunks new text
        odd = torch.repeat_interleave((torch.arange(count, device=dev) & 1).to(torch.bool), torch.from_numpy(np.diff(off).astype(np.int64)).to(dev))
        d_b = torch.where(odd, d_new, d_a)
        del odd
        cap = 2 * int(zk.lib.zk_compress_bound_list(n, count, 0))
        d_comp = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
        index = zk.DedupIndex(eng)
        c_off, d_d = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        snaps, wr_all = [], 0
        for d_src in (d_a, d_b):
            d_ids, d_fresh, d_cs, d_ds = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(4))
            torch.cuda.synchronize()
            m, wr = eng.encode_dedup_against_dev(index, d_comp, wr_all, u64(c_off), u64(d_d), len(c_off) - 1, d_src, d_off, count, 1, False,
                                                 d_comp.data_ptr() + wr_all, cap - wr_all, d_ids, d_fresh, d_cs, d_ds)
            c_off = np.concatenate([c_off, c_off[-1] + np.cumsum(d_cs[:m].cpu().numpy().view(np.uint32), dtype=np.uint64)])
            d_d = np.concatenate([d_d, d_d[-1] + np.cumsum(d_ds[:m].cpu().numpy().view(np.uint32), dtype=np.uint64)])
            wr_all += wr
            snaps.append((d_ids, d_src, m))
        nf = len(c_off) - 1
        d_c, d_dd = u64(c_off), u64(d_d)
        d_rel = u64(off - off[0])
        say(f"\n## avg_size {avg}: {count} chunks per snapshot; A stored {snaps[0][2]} frames, B {snaps[1][2]} more ({count - snaps[1][2]} of its chunks repeat); archive {nf} frames, {wr_all} bytes")
        one_o, one_l, zero = u64([int(off[0])]), u64([n]), u64([0])
        # snapshot C: every even chunk of A twice in a row -- half its chunks repeat chunks of its own; nothing needs storing for it
        ids_a = snaps[0][0].cpu().numpy().view(np.uint32)
        ids_c = ids_a[np.arange(count) & ~1]
        off_c = np.concatenate([[0], np.cumsum(np.diff(d_d)[ids_c], dtype=np.uint64)]).astype(np.uint64)
        n_c = int(off_c[-1])
        d_ids_c = torch.from_numpy(ids_c.view(np.int32).copy()).to(dev)
        d_off_c = u64(off_c)
        d_out_c = torch.empty(n_c + 64, dtype=torch.uint8, device=dev)
        d_ref_c = torch.empty(n_c + 64, dtype=torch.uint8, device=dev)
        one_lc = u64([n_c])

        def view_c():
            assert eng.read_view_ranges_dev(d_comp, wr_all, d_c, d_dd, nf, d_ids_c, d_off_c, count, zero, one_lc, zero, 1, d_out_c, n_c, False) == 0

        def listed_c():
            assert eng.decode_frame_list_dev(d_comp, wr_all, d_c, d_dd, d_ids_c, d_off_c, count, d_ref_c, n_c, False) == 0

        tv, frames = timed(view_c), eng.ranges_frames_decoded()
        tl = timed(listed_c)
        assert torch.equal(d_out_c[:n_c], d_ref_c[:n_c])
        p, g, d = parts(profiled(view_c), True)
        dl = sum(profiled(listed_c).get(k, 0.0) for k in DECODE)
        say(f"  restore of snapshot C ({n_c} bytes, every even chunk of A twice)")
        say(f"    frame list (parent)   {fmt(tl)}   {n_c / tl[0] / 1e6:.1f} GB/s; decode kernels {dl:.3f}")
        say(f"    one range of the view {fmt(tv)}   {n_c / tv[0] / 1e6:.1f} GB/s; {frames} distinct frames; profiled: plan {p:.3f}, gather {g:.3f}, decode kernels {d:.3f}")
        del d_out_c, d_ref_c
        for name, (d_ids, d_src, _) in zip("AB", snaps):
            def view():
                assert eng.read_view_ranges_dev(d_comp, wr_all, d_c, d_dd, nf, d_ids, d_off, count, one_o, one_l, zero, 1, d_out, n, False) == 0

            def listed():
                assert eng.decode_frame_list_dev(d_comp, wr_all, d_c, d_dd, d_ids, d_rel, count, d_out, n, False) == 0

            tv = timed(view)
            assert torch.equal(d_out[:n], d_src)
            frames = eng.ranges_frames_decoded()
            tl = timed(listed)
            assert torch.equal(d_out[:n], d_src)
            tc = timed(lambda: d_copy[:n].copy_(d_out[:n]))
            p, g, d = parts(profiled(view), True)
            dl = sum(profiled(listed).get(k, 0.0) for k in DECODE)
            say(f"  restore of snapshot {name} ({n} bytes)")
            say(f"    frame list (parent)   {fmt(tl)}   {n / tl[0] / 1e6:.1f} GB/s; decode kernels {dl:.3f}")
            say(f"    one range of the view {fmt(tv)}   {n / tv[0] / 1e6:.1f} GB/s; {frames} distinct frames; profiled: plan {p:.3f}, gather {g:.3f}, decode kernels {d:.3f}")
            say(f"    plain copy            {fmt(tc)}   gather / copy = {g / tc[0]:.2f}")
        # random reads through B's view, and the same shapes on the archive's own stream
        d_ids = snaps[1][0]
        total = int(d_d[-1])
        rng = np.random.default_rng(11)
        for k, size in ((1024, 4096), (65536, 4096), (16, 16 << 20)):
            if size * 2 > n:
                continue
            o_v = u64(int(off[0]) + rng.integers(0, n - size, k))
            o_a = u64(rng.integers(0, total - size, k))
            l = u64(np.full(k, size))
            res = {}

            def view():
                res["v"] = eng.read_view_ranges_dev(d_comp, wr_all, d_c, d_dd, nf, d_ids, d_off, count, o_v, l, None, k, d_out, min(k * size, n), False)

            def plain():
                res["a"] = eng.read_ranges_dev(d_comp, wr_all, d_c, d_dd, nf, o_a, l, None, k, d_out, min(k * size, n), False)

            if k * size > n:
                continue
            tv = timed(view)
            fv = eng.ranges_frames_decoded()
            ta = timed(plain)
            fa = eng.ranges_frames_decoded()
            assert res == {"v": 0, "a": 0}
            pv, pa = parts(profiled(view), True), parts(profiled(plain), False)
            say(f"  {k} ranges of {size} bytes")
            say(f"    zk_read_ranges_dev on the archive {fmt(ta)}   {fa} frames; profiled: plan {pa[0]:.3f}, gather {pa[1]:.3f}, decode kernels {pa[2]:.3f}")
            say(f"    through B's view                  {fmt(tv)}   {fv} frames; profiled: plan {pv[0]:.3f}, gather {pv[1]:.3f}, decode kernels {pv[2]:.3f}")
        index.close()
        del d_comp, d_b
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
