"""zk_encode_frames_dict_dev timed beside the plain and the prefix route: records (tests/helpers/dict_fixtures.py) HBM to HBM
at frame sizes 256 B, 1 KiB, 4 KiB and 64 KiB, level 1, no checksums, against the fixture's trained dictionary (its content as the prefix
of the prefix route).  Per route: ms (median of five calls after a warm-up), their spread, GiB/s of input and ratio; for the dictionary route
the per-kernel times of one profiled call; beside them libzstd 1.5.7 with the dictionary on one core (ZSTD_compress_usingCDict over a sample).
The input is 16 MiB of records tiled on the device.  Its size per frame size is capped so that no route reserves more than --scratch-gib of
per-frame scratch: the encoder keeps ~4 KiB of tables per frame, and the prefix route stages frames x (16 248 + frame size) bytes in one piece
(the dictionary route stages slices).  The prefix route's kernels are the parent commit's instruction for instruction (tools/kdiff.py), so
its row is the parent's figure of the same session.  No threshold.
usage: python tools/dict_encode_probe.py [--out profiles/dict_encode_probe.txt] [--gib 1] [--scratch-gib 8]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--scratch-gib", type=float, default=8.0)
    args = ap.parse_args()
    import torch
    import zeekstd_amd as zk
    from helpers import dict_fixtures as df
    from helpers import enc_dict_sim
    from oracle import libzstd_ref
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = zk.Engine(0)
    say(f"# tools/dict_encode_probe.py on {eng.device_name}")
    d = enc_dict_sim.fixture_dicts()["trained"]
    content = d[zk.Dictionary(d).content_offset:]
    cdict = zk.EncodeDictionary(eng, zk.Dictionary(d))
    sample = df.records(7001, 16 << 20)
    tile = torch.from_numpy(np.frombuffer(sample, np.uint8).copy()).to(dev)
    d_prefix = torch.from_numpy(np.frombuffer(content + bytes(64), np.uint8).copy()).to(dev)
    hist = len(content) & ~3

    def timed(fn):
        fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    z = libzstd_ref.load("1.5.7")
    for fs in (256, 1024, 4096, 65536):
        budget = int(args.scratch_gib * (1 << 30))
        frames = min(int(args.gib * (1 << 30)) // fs, budget // (hist + fs), budget // 4096)
        n = frames * fs
        d_src = tile.repeat(-(-n // tile.numel()))[:n].contiguous()
        cap = int(zk.lib.zk_compress_bound_dict(n, fs))
        d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        say(f"\n## frames of {fs} bytes: {frames} frames, {n / (1 << 20):.0f} MiB of input")
        routes = {
            "plain": lambda: eng.encode_frames_dev(d_src, n, fs, 1, False, d_dst, cap),
            "prefix": lambda: lib_prefix(zk, eng, d_src, n, fs, d_prefix, len(content), d_dst, cap),
            "dictionary": lambda: eng.encode_frames_dict_dev(d_src, n, fs, 1, False, cdict, d_dst, cap),
        }
        for name, fn in routes.items():
            nf, written = fn()
            med, lo, hi = timed(fn)
            say(f"  {name:<10} {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f})  {n / (1 << 30) / (med / 1e3):7.2f} GiB/s  ratio {n / written:.3f}")
        eng.set_profiling(True)
        routes["dictionary"]()
        times = eng.kernel_times()
        eng.set_profiling(False)
        say("  dictionary route by kernel: " + ", ".join(f"{k} {v:.2f}" for k, v in times.items() if v > 0))
        if z is not None:
            say("  " + cpu_figure(z, d, sample[:4 << 20], fs))
        del d_src, d_dst
    cdict.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def lib_prefix(zk, eng, d_src, n, fs, d_prefix, plen, d_dst, cap):
    nfo, wr = C.c_uint32(), C.c_uint64()
    L = zk.lib
    if L.zk_encode_frames_prefix_dev.argtypes is None:
        L.zk_encode_frames_prefix_dev.restype = C.c_int
        L.zk_encode_frames_prefix_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                  C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p]
    rc = L.zk_encode_frames_prefix_dev(eng._h, d_src.data_ptr(), n, fs, 1, 0, d_prefix.data_ptr(), plen, d_dst.data_ptr(), cap, None, None,
                                       C.byref(nfo), C.byref(wr), None)
    if rc:
        raise zk.ZkError(rc)
    return nfo.value, wr.value


def cpu_figure(z, dictionary, data, fs):
    """libzstd 1.5.7, level 1, one core, a compiled dictionary: MiB/s and ratio over `data` in frames of fs bytes"""
    z.ZSTD_createCDict.restype = C.c_void_p
    z.ZSTD_createCDict.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    z.ZSTD_compress_usingCDict.restype = C.c_size_t
    z.ZSTD_compress_usingCDict.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    z.ZSTD_freeCDict.argtypes = [C.c_void_p]
    cd = z.ZSTD_createCDict(dictionary, len(dictionary), 1)
    cctx = z.ZSTD_createCCtx()
    src = np.frombuffer(data, np.uint8)
    out = C.create_string_buffer(fs + 1024)
    total = 0
    t0 = time.perf_counter()
    for o in range(0, len(data), fs):
        total += z.ZSTD_compress_usingCDict(cctx, out, len(out), src.ctypes.data + o, min(fs, len(data) - o), cd)
    dt = time.perf_counter() - t0
    z.ZSTD_freeCCtx(cctx); z.ZSTD_freeCDict(cd)
    return f"libzstd 1.5.7 level 1 with the dictionary, one core (called from Python): {len(data) / (1 << 20) / dt:.0f} MiB/s, ratio {len(data) / total:.3f}"


if __name__ == "__main__":
    main()
