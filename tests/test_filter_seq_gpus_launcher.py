"""`katgpu filter seq --gpus N`: what the launcher decides before any rank touches a device.  `--gpus` is accepted for `filter` when the
sub-mode -- the first positional after `filter`, -v / --verbose / --help skipped, in any case -- is `seq`; `filter kmer` stays refused.
Without a device an accepted run forks its ranks and every one of them fails at katgpu_init."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")

pytestmark = pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK), reason="a GPU is visible")


def _run(args, cwd):
    return subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.fixture()
def inputs(tmp_path):
    (tmp_path / "x.fa").write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    (tmp_path / "y.fa").write_text(">g\nACGTACGTACGTACGTACGTACGTACGTACGTACGTTTGACA\n")
    return tmp_path


@pytest.mark.parametrize("args", [["filter", "seq", "--gpus", "2", "--seq", "x.fa", "y.fa"],
                                  ["filter", "SEQ", "--gpus=2", "--seq", "x.fa", "y.fa"],
                                  ["filter", "-v", "Seq", "--gpus", "2", "--seq", "x.fa", "y.fa"]])
def test_filter_seq_is_accepted_and_reaches_the_device(inputs, args):
    r = _run(args, inputs)
    assert "--gpus applies to" not in r.stderr, r.stderr[-2000:]
    assert r.returncode == 5 and "no gfx950 device" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert sorted(os.listdir(inputs)) == ["x.fa", "y.fa"]          # no rank created anything


def test_gpus_range_is_checked_first(inputs):
    r = _run(["filter", "seq", "--gpus", "300", "--seq", "x.fa", "y.fa"], inputs)
    assert r.returncode == 1 and "--gpus takes 1 .. 256" in r.stderr


def test_filter_alone_prints_its_usage(inputs):
    r = _run(["filter", "--gpus", "2"], inputs)
    assert r.returncode == 1 and "Usage: kat filter <mode>" in r.stdout and "--gpus applies to" not in r.stderr
    r = _run(["filter", "-v", "--gpus", "2"], inputs)
    assert r.returncode == 1 and "Usage: kat filter <mode>" in r.stdout


@pytest.mark.parametrize("sub", ["kmer", "KMER", "x"])
def test_other_sub_modes_stay_refused(inputs, sub):
    r = _run(["filter", sub, "--gpus", "2", "x.fa"], inputs)
    assert r.returncode == 1 and "--gpus applies to hist, gcp and comp" in r.stderr
    assert sorted(os.listdir(inputs)) == ["x.fa", "y.fa"]
