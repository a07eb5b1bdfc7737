"""bench.py as the driver runs it, on a small workload: a plain run prints the headline line alone, --steps sets the timed steps, and
--dump-outputs writes what the last timed step decoded -- the generator's bytes at the seeded positions, every frame's byte sum, zero
statuses -- as float arrays of at most 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_decoded_bytes(tmp_path):
    import bench
    from oracle import zko
    nframes, out = 16, tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(nframes), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "decode_decompressed_GiB_per_s" and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert not {"cpu_baseline", "roofline", "encode", "seek", "end_to_end"} & set(line)          # --full legs stay out of a plain run

    data = np.frombuffer(zko.gen_chunks(nframes * bench.FRAME, 0), np.uint8)
    sample = np.load(out / "decoded_sample.npy")
    sums = np.load(out / "decoded_frame_sums.npy")
    status = np.load(out / "frame_status.npy")
    assert sample.dtype == np.float32 and sums.dtype == np.float64 and status.dtype == np.float32
    assert np.array_equal(sample, data[bench.dump_positions(data.size)].astype(np.float32))
    assert np.array_equal(sums, data.reshape(nframes, -1).sum(1, dtype=np.int64).astype(np.float64))
    assert status.shape == (nframes,) and not status.any()
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
