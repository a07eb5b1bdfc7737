"""zk_frame_digests_dev and zk_archive_digests_dev timed beside the calls a chunk store already makes on the same list: --mib MiB
(1 GiB) of the bench's text (oracle/zko.gen_chunks) resident in HBM, cut by zk_chunk_boundaries_dev at avg_size 4 KiB, 64 KiB and 2 MiB (min =
avg / 4, max = 4 avg).  Per list and algorithm (SHA-256, the BLAKE2s tree), ms = median of --repeats calls after a warm-up (host clock around a
call that ends in a synchronise), GB/s = the list's bytes over that time:
  digests              zk_frame_digests_dev; from one profiled call the ms of its kernels: zk_k_digest_plan (leaf counts and their prefix sums),
                       zk_k_digest_leaves (the leaf pass, or SHA-256's frame pass), zk_k_digest_roots
and beside them, on the same list, the yardsticks -- the parent's calls, never the code under test:
  keys                 zk_frame_keys_dev (the additive 64-bit key the dedup index stores)
  copy                 a plain device copy of the list's bytes
  list encode          zk_encode_frame_list_dev, level 1, no checksums
and the ratios digests / keys, digests / copy, digests / list encode.  Then
  hashlib              one host core over a --host-mib (64) MiB slice cut by the same offsets: hashlib.sha256, and the tree by hashlib.blake2s
  archive              the 64 KiB list stored (zk_encode_frame_list_dev, checksums on): zk_archive_digests_dev over it per algorithm, beside
                       zk_dedup_index_add_archive_dev over the same archive (the decode and the key pass the digests replace)
No threshold is set anywhere: the numbers are reported as they come.
--digests-only times the digest calls alone; with ZEEKSTD_AMD_LIB naming a variant library (tools/build_digest_variant.sh: another slab size, four
waves per workgroup, the per-lane loader without a slab) that is how the alternatives to the chosen loader were measured.
usage: python tools/digest_probe.py [--out profiles/digest_probe.txt] [--repeats 5] [--mib 1024] [--host-mib 64] [--digests-only]"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALGOS = ("sha256", "blake2s-tree")


def tree(m, L=4096):
    n = max(1, -(-len(m) // L))
    inner = b"".join(hashlib.blake2s(m[k * L:(k + 1) * L], digest_size=32, fanout=0, depth=2, leaf_size=L, node_offset=k,
                                     node_depth=0, inner_size=32, last_node=(k == n - 1)).digest() for k in range(n))
    return hashlib.blake2s(inner, digest_size=32, fanout=0, depth=2, leaf_size=L, node_offset=0, node_depth=1,
                           inner_size=32, last_node=True).digest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--host-mib", type=int, default=64)
    ap.add_argument("--digests-only", action="store_true", help="the digest calls alone: a variant library (tools/build_digest_variant.sh) beside the built one")
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

    def row(name, t, nbytes, extra=""):
        say(f"    {name:<22}{t[0]:10.3f} ms  ({t[1]:.3f} .. {t[2]:.3f})  {nbytes / t[0] / 1e6:9.1f} GB/s{extra}")

    eng = zk.Engine(0)
    n = args.mib << 20
    say(f"# tools/digest_probe.py{' --digests-only, ' + os.path.basename(zk.LIB_PATH) if args.digests_only else ''} on {eng.device_name}: {args.mib} MiB of the bench's text in HBM; ms per call = median of {args.repeats} (min .. max)")
    host = np.frombuffer(zko.gen_chunks(n, 0), np.uint8)
    d_src = torch.from_numpy(host.copy()).to(dev)
    d_copy = torch.empty_like(d_src)
    stored = None
    for avg in (4 << 10, 64 << 10, 2 << 20):
        d_off = eng.chunk_boundaries_dev(d_src, n, avg_size=avg)
        off = d_off.cpu().numpy().view(np.uint64).astype(np.int64)
        count = len(off) - 1
        say(f"\n## avg_size {avg}: {count} chunks, mean {n / count:.0f} bytes, longest {int((off[1:] - off[:-1]).max())}")
        d_keys = torch.zeros(count, dtype=torch.int64, device=dev)
        d_dig = torch.zeros(count * 32, dtype=torch.uint8, device=dev)

        def digests(algo):
            """the call timed, then once more with the kernels' events"""
            t = timed(lambda: eng.frame_digests_dev(d_src, d_off, count, d_dig, algo))
            zk.lib.zk_engine_set_profiling(eng._h, 1)
            eng.frame_digests_dev(d_src, d_off, count, d_dig, algo)
            kt = {k: v for k, v in eng.kernel_times().items() if k.startswith("zk_k_digest")}
            zk.lib.zk_engine_set_profiling(eng._h, 0)
            row("digests " + algo, t, n, "   profiled: " + ", ".join(f"{k} {v:.3f}" for k, v in kt.items()))
            return t

        if args.digests_only:
            for algo in ALGOS:
                digests(algo)
            continue
        cap = int(zk.lib.zk_compress_bound_list(n, count, 0))
        d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        keys = timed(lambda: eng.frame_keys_dev(d_src, d_off, count, d_keys))
        copy = timed(lambda: d_copy.copy_(d_src))
        enc = timed(lambda: eng.encode_frame_list_dev(d_src, d_off, count, 1, False, d_dst, cap))
        row("keys", keys, n)
        row("copy", copy, n)
        row("list encode", enc, n)
        for algo in ALGOS:
            t = digests(algo)
            # a spot check of what was timed: the first, a middle and the last chunk against hashlib
            got = d_dig.cpu().numpy().reshape(count, 32)
            for i in (0, count // 2, count - 1):
                m = host[off[i]:off[i + 1]].tobytes()
                if got[i].tobytes() != (hashlib.sha256(m).digest() if algo == "sha256" else tree(m)):
                    raise SystemExit(f"{algo}: chunk {i} differs from hashlib")
            say(f"      / keys = {t[0] / keys[0]:.2f}   / copy = {t[0] / copy[0]:.2f}   / list encode = {t[0] / enc[0]:.3f}")
        if avg == 64 << 10:
            # the archive the last section digests: this list stored with checksums
            d_cs, d_ds = (torch.zeros(count, dtype=torch.int32, device=dev) for _ in range(2))
            wr = eng.encode_frame_list_dev(d_src, d_off, count, 1, True, d_dst, cap, d_cs, d_ds)
            c_off = np.concatenate([[0], np.cumsum(d_cs.cpu().numpy().view(np.uint32), dtype=np.uint64)]).astype(np.int64)
            stored = (d_dst[:wr + 64].clone(), wr, torch.from_numpy(c_off).to(dev), torch.from_numpy(off - off[0]).to(dev), count)
        del d_dst, d_keys, d_dig

    if args.digests_only:
        eng.close()
        if args.out:
            with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    hn = min(args.host_mib << 20, n)
    say(f"\n## one host core, hashlib over the first {hn >> 20} MiB cut at avg_size 65536")
    hoff = eng.chunk_boundaries_dev(d_src, hn, avg_size=64 << 10).cpu().numpy().view(np.uint64).astype(np.int64)
    for name, fn in (("sha256", lambda m: hashlib.sha256(m).digest()), ("blake2s-tree", tree)):
        t0 = time.perf_counter()
        for i in range(len(hoff) - 1):
            fn(host[hoff[i]:hoff[i + 1]].tobytes())
        ms = (time.perf_counter() - t0) * 1e3
        say(f"    {name:<22}{ms:10.1f} ms  {hn / ms / 1e6:9.3f} GB/s")

    d_comp, comp_size, d_c, d_d, count = stored
    say(f"\n## the stored archive: {count} frames, {comp_size} compressed bytes, {n} decoded")
    d_dig = torch.zeros(count * 32, dtype=torch.uint8, device=dev)

    def add_archive():
        x = zk.DedupIndex(eng)
        try:
            x.add_archive_dev(d_comp, comp_size, d_c, d_d, count)
        finally:
            x.close()

    add = timed(add_archive)
    row("index add_archive", add, n)
    for algo in ALGOS:
        t = timed(lambda: eng.archive_digests_dev(d_comp, comp_size, d_c, d_d, 0, count, d_dig, algo))
        row("archive digests " + algo[:7], t, n, f"   / add_archive = {t[0] / add[0]:.2f}")
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
