#!/usr/bin/env python3
"""zk_train_dictionary on the GPU, not a test: time per stage and the compressed totals for four inputs -- the dictionary fixture's samples at
16 KiB and at 110 KiB, the bench's input cut into 4 KiB samples, and random bytes -- and the 120 held-out frames of tests/test_gpu_train.py
against the fixture's libzstd-trained dictionary.  Writes profiles/dict_train_probe.txt."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zeekstd_amd as zk                                      # noqa: E402
from helpers import enc_dict_sim as S                         # noqa: E402
from helpers import train_model as M                          # noqa: E402
from oracle import zko                                        # noqa: E402


def total(engine, samples, dictionary=None):
    data, off = M.join(samples)
    cd = zk.EncodeDictionary(engine, zk.Dictionary(dictionary)) if dictionary else None
    comp, _ = engine.encode_frame_list(data, off, 1, False, dictionary=cd)
    if cd is not None:
        cd.close()
    return len(comp)


def main():
    out = open(os.path.join(ROOT, "profiles", "dict_train_probe.txt"), "w")

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line)
        out.write(line + "\n")
    e = zk.Engine(0)
    say("zk_train_dictionary on", e.device_name, "-- level 1, d = 8, f = 20, k = 0 (candidates 64 / 128 / 256 / 512); times in ms")
    say("wall: the whole host-pointer call (upload, count, select, an encode of the samples per candidate, one without a dictionary, the statistics,")
    say("the header); count / select / stats: the kernels alone (HIP events; select = all candidates side by side)")
    fixture = M.fixture_samples()
    text = zko.gen_chunks(8 << 20, 3)
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, 4 << 20, dtype=np.uint8).tobytes()
    cases = [("fixture samples, 16 KiB", fixture, 16384), ("fixture samples, 110 KiB", fixture, 112640),
             ("bench input, 8 MiB in 4 KiB samples, 110 KiB", [text[i:i + 4096] for i in range(0, len(text), 4096)], 112640),
             ("random bytes, 4 MiB in 4 KiB samples, 110 KiB", [noise[i:i + 4096] for i in range(0, len(noise), 4096)], 112640)]
    for name, samples, cap in cases:
        data, off = M.join(samples)
        e.train_dictionary(data, off, cap)                   # buffers grow on the first call
        e.set_profiling(True)
        t0 = time.perf_counter()
        d, rep = e.train_dictionary(data, off, cap, report=True)
        wall = (time.perf_counter() - t0) * 1e3
        kt = e.kernel_times()
        e.set_profiling(False)
        say("%-48s samples %8d bytes in %5d  wall %8.2f  count %6.3f  select %7.3f  stats %6.3f  k %3d  segments %4d  dictionary %6d bytes (header %3d)  "
            "samples encoded: %d without, %d against the content" % (name, rep["sample_bytes"], len(samples), wall, kt.get("zk_k_train_count", 0),
                                                                   kt.get("zk_k_train_select", 0), kt.get("zk_k_train_stats", 0), rep["k_chosen"],
                                                                   rep["segments"], len(d), rep["header_bytes"], rep["compressed_without"], rep["compressed_with"]))
        for k in (64, 128, 256, 512):
            e.set_profiling(True)
            e.train_dictionary(data, off, cap, k=k, raw_content=True)
            say("    k = %3d alone: select %7.3f ms" % (k, e.kernel_times().get("zk_k_train_select", 0)))
            e.set_profiling(False)
    held = M.held_out()
    trained = e.train_dictionary(fixture, None, 16384)
    raw = trained[zk.Dictionary(trained).content_offset:]
    fx = S.fixture_dicts()["trained"]
    fx_raw = fx[zk.Dictionary(fx).content_offset:]
    t = {"none": total(e, held), "fixture, content alone": total(e, held, fx_raw), "fixture (libzstd 1.5.7 ZDICT_trainFromBuffer)": total(e, held, fx),
         "trained, content alone": total(e, held, raw), "trained": total(e, held, trained)}
    say("held-out frames (120, 71 680 bytes) through Engine.encode_frame_list at level 1, bytes:")
    for k, v in t.items():
        say("    %-48s %6d" % (k, v))
    ref = t["fixture (libzstd 1.5.7 ZDICT_trainFromBuffer)"]
    say("    excess of the trained dictionary over the fixture's: %.2f %%  (the margin of tests/test_gpu_train.py: that, rounded up to a whole percent)"
        % (100.0 * (t["trained"] - ref) / ref))
    e.close()
    out.close()


if __name__ == "__main__":
    main()
