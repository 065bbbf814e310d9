"""Host side of the packed mode (no GPU): row offsets from an attention mask, the `pack_frames` config key, and the
C ABI additions - ca_pack_rows / ca_unpack_rows in header, SIGNATURES and library, and CaAttnDesc.row_off where the
header's compiler puts it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
KERNELS, STRIDES = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)


def test_row_offsets_from_a_host_attention_mask():
    """row_off == [0, cumsum(_get_feat_extract_output_lengths)] on ragged masks (one shorter than the first kernel,
    one full), as tests/test_kernels_gpu.py::test_frame_lengths states the lengths."""
    from coral_amd.wav2vec2 import frame_row_offsets

    N = 16000
    lens = torch.tensor([16000, 12345, 400, 7, 9999])
    mask = (torch.arange(N)[None, :] < lens[:, None]).long()
    n = lens.clone()
    for k, s in zip(KERNELS, STRIDES):
        n = torch.div(n - k, s, rounding_mode="floor") + 1
    flen, row_off = frame_row_offsets(mask, KERNELS, STRIDES)
    assert flen.tolist() == n.tolist()
    assert row_off.dtype == torch.int32 and row_off.tolist() == [0] + torch.cumsum(n, 0).tolist()
    # the valid-row share of a batch the issue quotes: eight clips of 303 ... 443 frames padded to 499
    frames = [303, 426, 142, 260, 411, 436, 318, 443]
    samples = torch.tensor([(f - 1) * 320 + 400 for f in frames])
    mask = (torch.arange(160000)[None, :] < samples[:, None]).int()
    flen, row_off = frame_row_offsets(mask, KERNELS, STRIDES)
    assert flen.tolist() == frames and int(row_off[-1]) == 2739


def test_pack_frames_config_key():
    from coral_amd.config import load_config

    base = ["model=test-wav2vec2", "datasets=synthetic"]
    assert load_config("asr_finetuning", base).pack_frames is False
    assert load_config("asr_finetuning", base + ["pack_frames=true"]).pack_frames is True
    line = [l for l in (ROOT / "config" / "asr_finetuning.yaml").read_text().splitlines() if l.startswith("pack_frames:")]
    assert line == ["pack_frames: false"]


def test_engine_switch_defaults_off(monkeypatch):
    """CA_PACK_FRAMES unset or 0 = off (read where the engine is built: no GPU needed to look at the rule)."""
    import inspect

    from coral_amd import wav2vec2

    src = inspect.getsource(wav2vec2.Wav2Vec2CTCEngine.__init__)
    assert 'os.environ.get("CA_PACK_FRAMES", "0") not in ("", "0")' in src


def test_pack_rows_symbols_agree():
    from coral_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "coral_amd.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in ("ca_pack_rows", "ca_unpack_rows"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        kinds = ["p" if "*" in a else a.split()[0] for a in args]
        assert kinds == ["p", "p", "p", "int32_t", "int32_t", "int32_t", "int32_t", "p"], (name, args)
        res, sig = _lib.SIGNATURES[name]
        assert res is C.c_int
        assert [("p" if t is C.c_void_p else {C.c_int32: "int32_t"}[t]) for t in sig] == kinds
        assert getattr(lib, name) is not None
        # argument validation needs no GPU
        assert getattr(lib, name)(None, None, None, 1, 1, 8, 2, None) == -1
        assert name.encode() in lib.ca_last_error()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
def test_attn_desc_layout_matches_the_header(tmp_path):
    """offsetof(CaAttnDesc, row_off) and sizeof(CaAttnDesc) as g++ lays the header out == the ctypes mirror; row_off is the
    last field, right behind split_ws_bytes."""
    from coral_amd._lib import CaAttnDesc

    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "coral_amd.h"\n'
                   'int main() { std::printf("%zu %zu %zu\\n", offsetof(CaAttnDesc, row_off), sizeof(CaAttnDesc), '
                   'offsetof(CaAttnDesc, split_ws_bytes)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-std=c++17", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    off, size, prev = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert off == CaAttnDesc.row_off.offset and size == C.sizeof(CaAttnDesc)
    assert prev == CaAttnDesc.split_ws_bytes.offset and off == prev + 8
    assert CaAttnDesc._fields_[-1][0] == "row_off" and CaAttnDesc._fields_[-2][0] == "split_ws_bytes"
