"""The GEMM kernel-choice rule (coral_amd/csrc/gemm_plan.h) without a GPU: tests/gemm_plan_check.cpp, built by the host
C++ compiler alone, must reproduce every field of every row of tests/golden/gemm_plan.json - recorded from the dispatcher
before the rule became a function of its own - and finds that the tile numbering covers every tile grid exactly once."""
import json
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "tests" / "golden" / "gemm_plan.json"


def test_gemm_plan_reproduces_the_recorded_dispatch(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "gemm_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "gemm_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(TABLE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = json.loads(TABLE.read_text())["rows"]
    assert f"{len(rows)} rows, 0 differ; tile cover ok" in r.stdout, r.stdout


def test_gemm_plan_table_covers_every_family_and_api():
    t = json.loads(TABLE.read_text())
    c = {k: i for i, k in enumerate(t["columns"])}
    assert 100 <= len(t["rows"]) <= 500
    assert {r[c["api"]] for r in t["rows"]} == {0, 1, 2}
    assert {r[c["family"]] for r in t["rows"] if not r[c["error"]]} == {0, 1, 2, 3, 4}
    assert {r[c["force_kernel"]] for r in t["rows"]} == {0, 1, 2, 3, 5}
    # beside a resident kernel (compute_cus below the device's count) the cost model gives each of its four answers
    tenant = [r for r in t["rows"] if 0 < r[c["compute_cus"]] < r[c["device_cus"]] and r[c["api"]] == 0 and r[c["force_kernel"]] == 0]
    assert {r[c["family"]] for r in tenant} >= {1, 2, 3, 4}
