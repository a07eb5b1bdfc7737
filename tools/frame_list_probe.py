"""zk_encode_frame_list_dev timed beside the uniform route over the same bytes: records (tests/helpers/dict_fixtures.py) HBM to
HBM, level 1, no checksums, one frame per record.  Record sizes are drawn evenly from 64..960 bytes (mean 512) at several record counts up to
half a million, and once from 2..6 KiB; routes: plain, and the dictionary route against the fixture's trained dictionary.  Per count and route:
  list, host plan      ZK_CHOICE_ENC_PLAN = 1: the frame / block / segment records written on the host and uploaded
  list, device plan    ZK_CHOICE_ENC_PLAN = 2: made on the device from the offsets (zk_enc_plan_dev.h)
  uniform              zk_encode_frames[_dict]_dev at frame_size = the mean: the code as it stood, the yardstick
each as the median of --repeats calls after a warm-up, the three taken in turn (host clock around a call that ends in a synchronise), then one
profiled call of each by kernel and what of the call lies outside every timed kernel.  The two plans' bytes are compared.  What
ZK_CHOICE_ENC_PLAN = 0 does from which count on (ZK_ENC_PLAN_DEV_FRAMES, zk_enc_plan.h) is read off this file.  No threshold here.
usage: python tools/frame_list_probe.py [--out profiles/frame_list_probe.txt] [--repeats 7]"""
import argparse
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--counts", default="1000,8000,64000,500000")
    args = ap.parse_args()
    import torch
    import zeekstd_amd as zk
    from helpers import dict_fixtures as df
    from helpers import enc_dict_sim
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = zk.Engine(0)
    say(f"# tools/frame_list_probe.py on {eng.device_name}: level 1, no checksums, ms per call = median of {args.repeats} (min .. max)")
    d = enc_dict_sim.fixture_dicts()["trained"]
    cdict = zk.EncodeDictionary(eng, zk.Dictionary(d))
    sample = df.records(7001, 16 << 20)
    tile = torch.from_numpy(np.frombuffer(sample, np.uint8).copy()).to(dev)

    def timed_in_turn(fns):
        for fn in fns.values():
            fn()
        ts = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    shapes = [(int(c), 64, 960) for c in args.counts.split(",")] + [(64000, 2048, 6144)]
    for count, lo, hi in shapes:
        rng = np.random.default_rng(count + lo)
        sizes = rng.integers(lo, hi + 1, count).astype(np.uint64)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        n = int(off[-1])
        mean = (lo + hi) // 2
        d_src = tile.repeat(-(-(n + 64) // tile.numel()))[:n + 64].contiguous()
        d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        say(f"\n## {count} records of {lo}..{hi} bytes: {n / (1 << 20):.1f} MiB of input; the uniform route cuts the same bytes every {mean}")
        for route, cd in (("plain", None), ("dictionary", cdict)):
            cap = max(int(zk.lib.zk_compress_bound_list(n, count, int(cd is not None))),
                      int(zk.lib.zk_compress_bound_dict(n, mean) if cd is not None else zk.lib.zk_compress_bound(n, mean)))
            d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)

            def list_call(plan):
                eng.set_kernel_choice(enc_plan=plan)
                return eng.encode_frame_list_dev(d_src, d_off, count, 1, False, d_dst, cap, dictionary=cd)

            def uniform_call():
                if cd is not None:
                    return eng.encode_frames_dict_dev(d_src, n, mean, 1, False, cd, d_dst, cap)[1]
                return eng.encode_frames_dev(d_src, n, mean, 1, False, d_dst, cap)[1]

            w1 = list_call(1)
            torch.cuda.synchronize()
            a = d_dst[:w1].clone()
            w2 = list_call(2)
            torch.cuda.synchronize()
            same = w1 == w2 and bool(torch.equal(a, d_dst[:w2]))
            del a
            wu = uniform_call()
            t = timed_in_turn({"list, host plan": lambda: list_call(1), "list, device plan": lambda: list_call(2), "uniform": uniform_call})
            say(f"  {route}: the two plans give {'the same' if same else 'DIFFERENT'} bytes; ratio list {n / w1:.3f}, uniform {n / wu:.3f}")
            for k, (med, mn, mx) in t.items():
                say(f"    {k:<18} {med:9.3f} ms  ({mn:.3f} .. {mx:.3f})  {n / (1 << 30) / (med / 1e3):7.2f} GiB/s  x{med / t['uniform'][0]:.3f} of uniform")
            say(f"    device plan - host plan: {t['list, device plan'][0] - t['list, host plan'][0]:+.3f} ms")
            eng.set_profiling(True)
            for plan, name in ((1, "list, host plan"), (2, "list, device plan"), (0, "uniform")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                list_call(plan) if plan else uniform_call()
                torch.cuda.synchronize()
                whole = (time.perf_counter() - t0) * 1e3
                times = {k: v for k, v in eng.kernel_times().items() if v > 0}
                say(f"    profiled, {name}: whole call {whole:.3f} ms; " + ", ".join(f"{k} {v:.3f}" for k, v in times.items()) +
                    f"; outside every timed kernel {whole - sum(times.values()):.3f}")
            eng.set_profiling(False)
            eng.set_kernel_choice(reset=0)
            del d_dst
        del d_src, d_off
    cdict.close()
    eng.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
