"""bench.py as it is run plainly (`--gpus 1 --steps K --warmup W`): the headline line without the --full legs, and
`--dump-outputs DIR`: what the last timed step returned, the same from run to run and equal to what the reference codec makes of
the benchmark's own frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES, STEPS = 640, 360, 4, 3


def run_plain(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                        "--frames", str(FRAMES), "--width", str(W), "--height", str(H), "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle_py
    from qoi_amd import synth

    out = run_plain(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == STEPS and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert abs(out["value"] - FRAMES * W * H / (out["ms_per_step"] * 1e-3) / 1e6) / out["value"] < 0.01
    for key in ("cpu_baseline", "cpu_baseline_all_cores", "single_frame", "other_content", "mixed_directory", "rgb_input"):
        assert key not in out, key
    assert out["reference_check"] is None and out["verified_bit_exact"] is None

    names = ("stream_lengths", "sample_frames", "streams_sample", "decoded_sample")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in names) <= 64 << 20

    # the benchmark's frames are synth's photo frames 0 .. FRAMES-1: streams byte for byte the reference encoder's, pixels the source's
    oracle = oracle_py.load_ref() or oracle_py.load_port()
    px = [synth.frame_rgba("photo", W, H, f).reshape(-1) for f in range(FRAMES)]
    want = [oracle.encode(p, W, H, 4) for p in px]
    assert a["stream_lengths"].tolist() == [len(s) for s in want]
    frames, pos, offs = bench.dump_sample(FRAMES, [len(s) for s in want], W * H)
    assert a["sample_frames"].tolist() == frames.tolist()
    for i, f in enumerate(frames):
        assert np.array_equal(a["streams_sample"][i], np.frombuffer(want[f], dtype=np.uint8)[pos[i]])
        assert np.array_equal(a["decoded_sample"][i], px[f][offs])

    # same arguments, same inputs, same outputs
    run_plain(tmp_path / "b")
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")), n
