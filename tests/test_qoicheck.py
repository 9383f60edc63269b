"""tools/qoicheck_mi355x.py on the GPU (-m gpu): one inspect_streams call over a set of .qoi files, a row per file, exit status 1
when a file is flagged."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flagged_file_sets_the_exit_status(tmp_path, ref, port):
    from qoi_amd import synth
    oracle = ref or port
    a = oracle.encode(synth.frame_rgba("photo", 64, 48, 0).reshape(-1), 64, 48, 4)
    b = oracle.encode(synth.frame_rgb("uiflat", 257, 9, 1).reshape(-1), 257, 9, 3)
    (tmp_path / "a.qoi").write_bytes(a)
    (tmp_path / "b.qoi").write_bytes(b)
    cut = tmp_path / "cut"
    cut.mkdir()
    (cut / "c.qoi").write_bytes(a[:-20])
    tool = [sys.executable, os.path.join(ROOT, "tools", "qoicheck_mi355x.py")]
    r = subprocess.run(tool + [str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.stdout, r.stderr)
    rows = {l.split()[0]: l for l in r.stdout.splitlines() if l.strip()}
    assert "PIXELS_SHORT" in rows["c.qoi"] and "64x48x4" in rows["c.qoi"]
    assert rows["a.qoi"].rstrip().endswith("-") and rows["b.qoi"].rstrip().endswith("-") and "257x9x3" in rows["b.qoi"]
    assert "1 flagged" in rows["total:"]
    r = subprocess.run(tool + [str(tmp_path / "a.qoi"), str(tmp_path / "b.qoi")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
