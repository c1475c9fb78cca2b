"""`katgpu hist` and `katgpu comp` on .jf inputs under `--gpus 2`: every rank loads its stretch of each file's records
(katgpu_jf_load_part) and the tables are made one by owner; the files written are the single-rank run's, byte for byte.
The two ranks share this box's one device over the /dev/shm transport, as the --gpus cases of tests/test_gpu_cli.py do."""
import os
import subprocess

import pytest

from kat_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")


def go(args, cwd, env):
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (args, r.stdout[-1500:], r.stderr[-3000:])
    return r


@pytest.mark.parametrize("k", [27, 41])
def test_jf_inputs_under_gpus_2(engine, tmp_path, k):
    g = synth.genome(30000, seed=20261017)
    for name, stream in (("a.jf", synth.reads(g, 0, 3000, seed=1)), ("b.jf", synth.stream_of_contigs(g, 5000))):
        t = engine.table(k, True, size_hint=1 << 14).count_bases(stream)
        t.dump_jf(str(tmp_path / name))
        t.free()
    plain = dict(os.environ)
    many = dict(plain, KATGPU_COMM_TRANSPORT="shm")
    many.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    many.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    m = "-m%d" % k
    go(["hist", m, "-o", "one.hist", "a.jf"], tmp_path, plain)
    go(["comp", m, "-o", "one", "a.jf", "b.jf"], tmp_path, plain)
    r = go(["hist", "--gpus", "2", m, "-o", "many.hist", "a.jf"], tmp_path, many)
    assert "Multi-GPU: 2 ranks, transport shm" in r.stdout
    go(["comp", "--gpus", "2", m, "-o", "many", "a.jf", "b.jf"], tmp_path, many)
    for a, b in (("one.hist", "many.hist"), ("one-main.mx", "many-main.mx"), ("one.stats", "many.stats")):
        x, y = (tmp_path / a).read_bytes(), (tmp_path / b).read_bytes()
        assert len(x) > 100 and x.replace(b"one", b"many") == y.replace(b"one", b"many"), (a, b)
