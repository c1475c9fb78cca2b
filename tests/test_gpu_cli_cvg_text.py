"""`katgpu sect` without -n on one GPU, with KATGPU_SECT_DEVICE_TEXT=1: the lines of -counts.cvg come from the device
(katgpu_table_record_cvg_text_host), the statistics and regions from the kernels `sect -n` uses, and no per-position profile crosses
the bus -- the runs here forbid katgpu_table_profile_host.  Every output is, byte for byte, what the per-position path writes: `--gpus 1` keeps that path (the counts
gathered on rank 0, every output made from them on the host), so its files are the yardstick; -counts.cvg is the oracle's as well.
Inputs: the tiny assembly and read pair of tests/test_gpu_cli_gathered_profile.py."""
import os

import pytest

from tests.test_gpu_cli_gathered_profile import _env, _go, tiny  # noqa: F401  (tiny: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [27, 41])
@pytest.mark.parametrize("opts", [[], ["-g"], ["-E", "-F", "-M", "2", "-G", "5"], ["-N"]], ids=["plain", "g", "EF", "N"])
def test_sect_without_n_needs_no_profile(tiny, ko, tmp_path, opts, k):  # noqa: F811
    asm, reads = str(tiny / "asm.fa"), [str(tiny / "pair_R1.fq"), str(tiny / "pair_R2.fq")]
    args = opts + ["-m", str(k), "-o", "out", asm] + reads
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_TEST_FORBID_PROFILE_HOST="1", KATGPU_SECT_DEVICE_TEXT="1")
    r = _go(["sect"] + args, str(tmp_path / "device"), env)
    assert r.stderr.count('"phase": "sect_coverage"') == 1
    _go(["sect", "--gpus", "1"] + args, str(tmp_path / "gathered"), _env())
    device, gathered = sorted(os.listdir(tmp_path / "device")), sorted(os.listdir(tmp_path / "gathered"))
    assert device == gathered, (device, gathered)                    # every output, and no stray file
    assert len(device) == 2 + ("-g" in opts) + 2 * ("-E" in opts) and "out-counts.cvg" in device and "out-stats.tsv" in device, device
    for name in device:
        a, b = (tmp_path / "device" / name).read_bytes(), (tmp_path / "gathered" / name).read_bytes()
        assert a == b, name
        assert len(a) > 0, name
    canonical = "-N" not in opts
    table = (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_files(reads)
    ko.sect(table, asm, str(tmp_path / "want"), output_gc_stats="-g" in opts, extract_nr="-E" in opts, extract_r="-E" in opts, min_repeat=2,
            max_repeat=5 if "-E" in opts else 0)
    cvg = (tmp_path / "device" / "out-counts.cvg").read_bytes()
    assert cvg == (tmp_path / "want-counts.cvg").read_bytes()
    lines = cvg.split(b"\n")
    assert lines[0] == b">contig0 some words" and lines[3] == b"0" and len(lines) == 9     # (the contig shorter than k has no window)
    assert max(int(x) for x in lines[1].split()) >= 2 and lines[5].count(b" 0 ") >= 60      # coverage; the windows over the runs of N
