"""ca_overlap_merge is declared in the header, listed in the signature table and exported by the built library."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "coral_amd" / "libcoral_amd.so"


def test_the_symbol_is_declared_with_the_arguments_the_table_lists():
    from coral_amd import _lib

    header = (ROOT / "include" / "coral_amd.h").read_text()
    m = re.search(r"\bint ca_overlap_merge\(([^;]*)\);", header)
    assert m, "ca_overlap_merge is not declared in include/coral_amd.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["ca_overlap_merge"]
    assert res is ctypes.c_int and len(args) == len(params) == 16
    for p, a in zip(params, args):
        want = ctypes.c_void_p if "*" in p else (ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32)
        assert a is want, (p, a)
    assert re.search(r"#define CA_CHUNK_MERGE_MAX_TOKENS\s+1024\b", header) and _lib.CHUNK_MERGE_MAX_TOKENS == 1024
    assert "csrc/chunk_merge.hip" in header and (ROOT / "coral_amd" / "csrc" / "chunk_merge.hip").exists()


@pytest.mark.skipif(not LIB.exists(), reason="needs the built library")
def test_the_built_library_exports_the_symbol():
    from coral_amd import _lib, ops

    lib = _lib.load()
    assert lib.ca_overlap_merge.argtypes == _lib.SIGNATURES["ca_overlap_merge"][1]
    assert callable(ops.overlap_merge) and callable(ops.overlap_merge_read) and callable(ops.skip_bitmap)
    # the argument checks answer without a device: a null pointer is CA_ERR_ARG with the function's name
    assert lib.ca_overlap_merge(None, 1, None, None, 1, 1, None, 0, None, None, 1, None, 1, None, None, None) == -1
    assert b"ca_overlap_merge" in lib.ca_last_error()
