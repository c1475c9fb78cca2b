"""`katgpu hist -d` writes its hash through the device-side .jf record producer: the same file as the host writer's."""
import os
import subprocess

import pytest

import kat_amd
from tests import jf_order_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")


def test_hist_dump(engine, refdata, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                  # the header records the working directory
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    r = subprocess.run([EXE, "hist", "-m27", "-d", "-o", "d.hist", r1], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    t = engine.table(27, True).count_files([r1])
    keys, counts = t.export()
    kat_amd.jf_write_records("want.jf27", 27, True, keys, counts)
    hdr_a, head_a, body_a = model.split("want.jf27")
    hdr_b, head_b, body_b = model.split("d.hist-hash.jf27")
    assert keys.size > 1000 and len(body_b) == keys.size * 11
    assert model.blank_time(head_a) == model.blank_time(head_b)
    assert body_a == body_b
    t.free()
