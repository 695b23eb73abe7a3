"""The LUT family primitive at the C boundary, without a GPU (sgfhe_bootstrap_lut_multi_batch, include/sgfhe_hip.h):
the header, the library and the ctypes binding agree on the symbol, its argument count and SGFHE_LUT_MAX_TABLES; the
ABI revision is unchanged (a function was added, none changed); a NULL ctx is refused before anything else is read.
The bytes are held to the oracle on the device in tests/test_gpu_lut_multi.py."""

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sgfhe_hip.h")
NAME = "sgfhe_bootstrap_lut_multi_batch"


def _prototypes():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(sgfhe_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, re.S)}


def test_header_library_and_binding_agree(S):
    protos = _prototypes()
    assert NAME in protos and NAME in S.EXPORTED_SYMBOLS
    L = S.lib()
    fn = getattr(L, NAME)
    assert len(fn.argtypes) == len(protos[NAME].split(",")) == 8
    # the single-table call it extends: the same arguments plus n_tables
    assert len(L.sgfhe_bootstrap_lut_batch.argtypes) == 7
    hdr = open(HDR).read()
    assert int(re.search(r"#define SGFHE_LUT_MAX_TABLES (\d+)u", hdr).group(1)) == 256 == S.engine.LUT_MAX_TABLES


def test_abi_revision_is_unchanged(S):
    assert S.ABI_VERSION == 7 == S.lib().sgfhe_abi_version()
    assert re.search(r"#define SGFHE_ABI_VERSION 7u?\b", open(HDR).read())


def test_null_ctx_is_invalid_arg(S):
    L = S.lib()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n_tables, batch in ((1, 0), (1, 1), (0, 1), (257, 1)):
        assert L.sgfhe_bootstrap_lut_multi_batch(None, p, p, p, n_tables, batch, p, 0) == -1   # SGFHE_ERR_INVALID_ARG
    assert all(x == 0 for x in buf)
