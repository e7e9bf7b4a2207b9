"""CPU: bench.py's command line has --full and --dump-outputs, and the dump
writer keeps its formats and its size budget.  bench.py sets the process's HIP
queue count when it is imported, so it is only ever loaded in a child."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import torch
import bench
n, out = int(sys.argv[1]), sys.argv[2]
g = torch.Generator().manual_seed(5)
rcs = [torch.randint(0, 3, (n,), dtype=torch.uint8, generator=g) for _ in range(4)]
torch.save(rcs, out + ".pt")
bench.dump_outputs(out, rcs, [{"n_commit": 3 + i, "n_abort": n - 3 - i} for i in range(4)])
"""


def _dump(tmp_path, name, n):
    out = str(tmp_path / name)
    subprocess.run([sys.executable, "-c", CHILD, str(n), out], cwd=ROOT, check=True, timeout=120)
    import torch
    return out, [t.numpy() for t in torch.load(out + ".pt")]


def test_options_present():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout and "--steps" in p.stdout


def test_dump_whole_outputs(tmp_path):
    n = 5000
    out, rcs = _dump(tmp_path, "small", n)
    assert sorted(os.listdir(out)) == ["counts.npy"] + [f"rc_lane{i}.npy" for i in range(4)]
    for i in range(4):
        a = np.load(os.path.join(out, f"rc_lane{i}.npy"))
        assert a.dtype == np.float32 and np.array_equal(a, rcs[i].astype(np.float32))
    c = np.load(os.path.join(out, "counts.npy"))
    assert c.dtype == np.float64 and c.tolist() == [[3 + i, n - 3 - i] for i in range(4)]


def test_dump_samples_within_budget(tmp_path):
    n = 1 << 23  # 4 lanes x 4 B x 8M txns = 128 MiB unsampled
    out, rcs = _dump(tmp_path, "big", n)
    files = os.listdir(out)
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 << 20
    idx = np.load(os.path.join(out, "sample_idx.npy"))
    assert idx.dtype == np.float64
    idx = idx.astype(np.int64)
    assert (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < n and idx.size > n // 4
    for i in range(4):
        a = np.load(os.path.join(out, f"rc_lane{i}.npy"))
        assert a.dtype == np.float32 and np.array_equal(a, rcs[i][idx].astype(np.float32))
    # the sample is fixed: a second dump picks the same txns
    out2, _ = _dump(tmp_path, "big2", n)
    assert np.array_equal(np.load(os.path.join(out2, "sample_idx.npy")).astype(np.int64), idx)
