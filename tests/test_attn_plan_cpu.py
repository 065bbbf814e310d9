"""The attention kernel-choice rule (coral_amd/csrc/attn_plan.h) without a GPU: tests/attn_plan_check.cpp, built by the
host C++ compiler alone, must reproduce every field of every row of tests/golden/attn_plan.json - recorded from the
dispatcher before the rule became a function of its own - and finds that the grid numbering covers every
(tile, head, clip) exactly once."""
import json
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "tests" / "golden" / "attn_plan.json"
CSRC = ROOT / "coral_amd" / "csrc"
INST = ("kernel", "hdpv", "drop", "wpe", "dt", "qp", "ks")


def test_attn_plan_reproduces_the_recorded_dispatch(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "attn_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "attn_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(TABLE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = json.loads(TABLE.read_text())["rows"]
    assert f"{len(rows)} rows, 0 differ; tile cover ok" in r.stdout, r.stdout


def _launcher_instantiations():
    """The `case attn_inst(KERNEL, hdpv, drop[, wpe, dt, qp, ks])` labels of the three launchers."""
    enum = re.search(r"enum AttnKernel \{(.*?)\};", (CSRC / "attn_plan.h").read_text(), re.S).group(1)
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"(ATTN_\w+) = (\d+)", enum)}
    found = set()
    for f in ("attn_fwd.hip", "attn_decode.hip", "attn_bwd.hip"):
        for m in re.finditer(r"case attn_inst\((ATTN_\w+)((?:, \d+)+)\):", (CSRC / f).read_text()):
            args = [int(x) for x in m.group(2).split(",")[1:]]
            found.add((ids[m.group(1)], *(args + [0] * 6)[:6]))
    return ids, found


def test_attn_plan_table_covers_every_instantiation_api_and_threshold():
    t = json.loads(TABLE.read_text())
    c = {k: i for i, k in enumerate(t["columns"])}
    rows = [{k: r[i] for k, i in c.items()} for r in t["rows"]]
    ok = [r for r in rows if not r["error"]]
    assert 100 <= len(rows) <= 400
    # every kernel id and every instantiation the launchers name - and nothing they do not
    ids, named = _launcher_instantiations()
    planned = {tuple(r[f"{k}{s}"] for k in INST) for r in ok for s in range(3) if r[f"kernel{s}"]}
    assert planned == named and {p[0] for p in planned} == set(ids.values()) - {0}, (planned ^ named)
    assert {r["api"] for r in ok} == {0, 1, 2}
    assert {r["error"] for r in rows} == {0, 1, 2, 3, 4}
    assert any(r["error"] == 2 and r["Tq"] < 100 for r in rows)  # O8 with too few queries
    assert {r["api"] for r in rows if r["error"] == 3} == {0, 1}  # a short split workspace in both decode entry points
    # both sides of every threshold, under default knobs
    dflt = [r for r in ok if (r["wide"], r["wpe3"], r["dq_wpe3"], r["dkv_wide"], r["dkv_wpe3"], r["smallq_2percu"], r["split"],
                               r["split_tail"]) == (1, 1, 1, 1, 0, -1, 4, 1)]
    d256 = [r for r in dflt if r["device_cus"] == 256]
    for api, side, slot, wide_kernel in ((0, "Tq", 0, 2), (2, "Tq", 1, 8), (2, "Tk", 2, 6)):
        for hd in (64, 72, 128):
            got = {(r[side], r[f"kernel{slot}"] == wide_kernel) for r in d256 if r["api"] == api and r["hd"] == hd and r[side] in (99, 100)}
            want_wide = not (wide_kernel == 6 and hd > 64)  # the 128-key dK|dV kernel is for head_dim <= 64
            assert got == {(99, False), (100, want_wide)}, (api, side, hd, got)
    assert {(r["Tq"], r["kernel0"]) for r in d256 if r["api"] == 0 and r["Tq"] in (16, 17) and r["hd"] == 64 and not r["causal"]
            and not r["row_off"] and not r["drop"]} == {(16, 3), (17, 1)}
    assert {(r["Tk"], r["nsplit"] > 1) for r in d256 if r["ws"] == 1 and r["B"] * r["H"] == 128 and r["Tk"] in (1023, 1024)} == \
        {(1023, False), (1024, True)}
    assert {(r["grid0"], r["dt0"]) for r in d256 if r["kernel0"] == 3 and r["grid0"] in (383, 384)} == {(383, 3), (384, 2)}
    # the three key-split regimes: at most one item per CU, a partly filled second round, two rounds or more
    split = [r for r in d256 if r["ws"] == 1 and r["Tk"] >= 1024 and r["kernel0"] == 3]
    assert any(r["B"] * r["H"] <= 256 and r["ns"] > 1 for r in split)
    assert any(256 < r["B"] * r["H"] < 512 and r["ns_tail"] > 1 and r["tail_start"] == 256 for r in split)
    assert any(r["B"] * r["H"] >= 512 and r["nsplit"] == 1 for r in split)
    # dropout, causal, klen, row_off; odd heads x clips
    for flag in ("drop", "causal", "klen", "row_off", "key_slot", "O8"):
        assert {r[flag] for r in ok} == {0, 1}, flag
    assert any((r["B"] * r["H"]) % 8 for r in ok if r["kernel0"] in (1, 2))
    # each knob at a value that is not its default, and a second device size
    for knob, default in (("wide", 1), ("wpe3", 1), ("dq_wpe3", 1), ("dkv_wide", 1), ("dkv_wpe3", 0), ("smallq_2percu", -1), ("split", 4),
                          ("split_tail", 1), ("device_cus", 256)):
        assert len({r[knob] for r in ok}) >= 2 and default in {r[knob] for r in ok}, knob
