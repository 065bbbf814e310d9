"""The per-row first key (CaAttnDesc.kstart) in the attention kernel-choice rule (coral_amd/csrc/attn_plan.h), without a
GPU: tests/attn_kstart_plan_check.cpp, built by the host C++ compiler alone, finds that a descriptor without kstart gets
the plan and the instantiation number it had, that kstart picks the km instantiations of the causal 64-query, the causal
128-query and the single-query kernel, and that every refused combination returns the plan error of its own.  The
launchers name exactly the km instantiations the rule can pick."""
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "coral_amd" / "csrc"


def test_attn_plan_with_and_without_kstart(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "attn_kstart_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "attn_kstart_plan_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unmasked descriptors unchanged; kstart forms and refusals ok" in r.stdout, r.stdout


def test_launchers_name_the_km_instantiations():
    """`case attn_inst(KERNEL, hdpv, drop, wpe, dt, qp, ks, 1)`: the 64-query kernel, the 128-query kernel at two and
    three workgroups per CU, the single-query kernel with rings of three and two - all at the head-dim image 64 without
    dropout, query projection or key_slot table - and no backward kernel."""
    found = set()
    for f in ("attn_fwd.hip", "attn_decode.hip", "attn_bwd.hip"):
        for m in re.finditer(r"case attn_inst\((ATTN_\w+)((?:, \d+){7})\):", (CSRC / f).read_text()):
            args = tuple(int(x) for x in m.group(2).split(",")[1:])
            assert args[-1] == 1, m.group(0)
            found.add((m.group(1), *args[:-1]))
    assert found == {("ATTN_FWD", 64, 0, 0, 0, 0, 0), ("ATTN_FWD_WIDE", 64, 0, 3, 0, 0, 0), ("ATTN_FWD_WIDE", 64, 0, 2, 0, 0, 0),
                     ("ATTN_FWD_SMALLQ", 64, 0, 0, 3, 0, 0), ("ATTN_FWD_SMALLQ", 64, 0, 0, 2, 0, 0)}, found


def test_python_mirror_has_kstart_behind_key_slot_and_null_by_default(tmp_path):
    """kstart stands with the pointers it belongs to, behind klen and key_slot, where the header has it (row_off stays the
    last field: tests/test_packed_cpu.py); the mirror's offset is the host compiler's."""
    import ctypes as C

    from coral_amd._lib import CaAttnDesc

    names = [f[0] for f in CaAttnDesc._fields_]
    assert names[names.index("key_slot") + 1] == "kstart" and names[-1] == "row_off"
    assert dict(CaAttnDesc._fields_)["kstart"] is C.c_void_p and CaAttnDesc().kstart is None
    assert CaAttnDesc.kstart.offset == CaAttnDesc.key_slot.offset + 8
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "coral_amd.h"\n'
                   'int main() { std::printf("%zu %zu\\n", offsetof(CaAttnDesc, kstart), sizeof(CaAttnDesc)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cxx, "-std=c++17", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    off, size = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert off == CaAttnDesc.kstart.offset and size == C.sizeof(CaAttnDesc)
