"""`katgpu cold --gpus N` and `katgpu sect -n --gpus N`: the statistics of every record and the regions of -E / -F come from
katgpu_table_record_stats_gathered_host -- the counts gathered on rank 0's device and reduced there -- and the lines of -g from the
bases alone.  With both per-position host paths forbidden (KATGPU_TEST_FORBID_PROFILE_GATHERED, KATGPU_TEST_FORBID_PROFILE_HOST)
every file of the multi run is the plain run's, byte for byte, and rank 0's record_stats_gathered lines say what came back.
`sect --gpus N` without -n still gathers the per-position counts: the hook stops it.  The inputs, environment and comparisons are
tests/test_gpu_cli_gathered_profile.py's."""
import json
import os
import re
import subprocess

import pytest

from tests.test_gpu_cli_gathered_profile import EXE, _env, _go, _jf, tiny  # noqa: F401  (tiny: the module-scoped fixture)

pytestmark = pytest.mark.gpu
STATS = re.compile(r'katgpu_timing (\{"phase": "record_stats_gathered".*\})')
GATHER = re.compile(r'katgpu_timing \{"phase": "profile_gathered"')
HOOK = "katgpu_table_profile_gathered_host is forbidden (KATGPU_TEST_FORBID_PROFILE_GATHERED)"


def _forbidding():
    return dict(_env(), KATGPU_TEST_FORBID_PROFILE_GATHERED="1", KATGPU_TEST_FORBID_PROFILE_HOST="1")


def _regions(path):
    """the regions of a -non_repetitive.fa / -repetitive.fa file: one header line each"""
    return sum(1 for ln in open(path, "rb") if ln.startswith(b">"))


# mode, options, k, ranks, the collective calls of a run (the assembly is one batch of records)
@pytest.mark.parametrize("mode,opts,k,gpus,calls", [
    ("cold", [], 27, 2, 2),
    ("cold", ["-d"], 27, 3, 2),
    ("sect", ["-n", "-g", "-E", "-F", "-M", "2", "-G", "5"], 27, 3, 1),
    ("sect", ["-n"], 41, 2, 1)])
def test_no_per_position_count_reaches_the_host(tiny, tmp_path, mode, opts, k, gpus, calls):  # noqa: F811
    args = opts + ["-m", str(k), "-o", "out", str(tiny / "asm.fa"), str(tiny / "pair_R1.fq"), str(tiny / "pair_R2.fq")]
    _go([mode] + args, str(tmp_path / "plain"), _env())
    r = _go([mode, "--gpus", str(gpus)] + args, str(tmp_path / "multi"), _forbidding())
    plain, multi = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(tmp_path / "multi"))
    assert plain == multi, (plain, multi)                            # every output, and no stray file
    assert "out-stats.tsv" in plain and "out-counts.cvg" not in plain
    assert len(plain) == 1 + ("-g" in opts) + 2 * ("-E" in opts) + ("-d" in opts) * 2, plain
    for name in plain:
        a, b = tmp_path / "plain" / name, tmp_path / "multi" / name
        if ".jf" in name:
            assert _jf(a) == _jf(b), name
        else:
            assert a.read_bytes() == b.read_bytes(), name
            assert a.stat().st_size > 0, name
    lines = [json.loads(x) for x in STATS.findall(r.stderr)]
    assert len(lines) == calls and len(GATHER.findall(r.stderr)) == calls, r.stderr[-3000:]
    n_regions = 0
    if "-E" in opts:
        n_regions = _regions(tmp_path / "plain" / "out-non_repetitive.fa") + _regions(tmp_path / "plain" / "out-repetitive.fa")
        assert n_regions > 0
    for t in lines:
        assert t == {"phase": "record_stats_gathered", "batches": 1, "ranks": gpus, "records": 4, "regions": n_regions, "back_bytes": 48 * 4 + 24 * n_regions}, lines


def test_sect_without_n_still_gathers_per_position(tiny, tmp_path):  # noqa: F811
    args = ["-m", "27", "-o", "out", str(tiny / "asm.fa"), str(tiny / "pair_R1.fq"), str(tiny / "pair_R2.fq")]
    env = _forbidding()
    os.makedirs(tmp_path / "stopped", exist_ok=True)
    r = subprocess.run([EXE, "sect", "--gpus", "2"] + args, cwd=tmp_path / "stopped", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and HOOK in r.stderr, (r.returncode, r.stderr[-3000:])
    _go(["sect", "--gpus", "2"] + args, str(tmp_path / "goes"), _env())
    assert (tmp_path / "goes" / "out-counts.cvg").stat().st_size > 0
