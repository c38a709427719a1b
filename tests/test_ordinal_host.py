"""Ordinals on the key index, host side, no GPU: the header's declarations, the
library's exports, null arguments, the Python names and the CLI's
--lookup-as argument."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "partitionedhashjoin_amd")
LIB = os.path.join(PKG, "libphj_hip.so")
CLI = os.path.join(PKG, "phjoin")
CALLS = ["phj_index_build_ex", "phj_index_flags_get", "phj_index_uniques", "phj_index_encode", "phj_index_accumulate"]
PHJ_ERR_INVALID = -1


def header():
    with open(os.path.join(ROOT, "include", "phj.h")) as f:
        return f.read()


def test_header_declares_the_calls_and_the_flag():
    text = header()
    for name in CALLS:
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
    assert re.search(r"^#define PHJ_INDEX_ORDINALS 0x1\b", text, flags=re.M)
    assert re.search(r"^#define PHJ_ABI_VERSION 2\b", text, flags=re.M)


def test_symbols_are_exported_and_listed():
    from partitionedhashjoin_amd import _capi
    lib = ctypes.CDLL(LIB)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTED, name
    assert _capi.INDEX_ORDINALS == 1
    assert ctypes.sizeof(_capi.IndexInfo) == 40


def test_null_context_or_index_is_invalid():
    lib = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    flags, n, ptr, h = ctypes.c_uint32(7), ctypes.c_uint64(7), P(), P()
    for f in CALLS:
        getattr(lib, f).restype = ctypes.c_int
    lib.phj_index_build_ex.argtypes = [P, P, ctypes.c_uint32, P, P]
    lib.phj_index_flags_get.argtypes = [P, P]
    lib.phj_index_uniques.argtypes = [P, P, P, P]
    lib.phj_index_encode.argtypes = [P, P, P, ctypes.c_uint32, ctypes.c_uint64, P, P, P]
    lib.phj_index_accumulate.argtypes = [P, P, P, ctypes.c_uint32, P, ctypes.c_uint32, ctypes.c_uint64, P, P, P]
    assert lib.phj_index_build_ex(None, None, 1, ctypes.byref(h), None) == PHJ_ERR_INVALID
    assert lib.phj_index_flags_get(None, ctypes.byref(flags)) == PHJ_ERR_INVALID
    assert lib.phj_index_uniques(None, None, ctypes.byref(ptr), ctypes.byref(n)) == PHJ_ERR_INVALID
    assert lib.phj_index_encode(None, None, None, 1, 0, None, None, None) == PHJ_ERR_INVALID
    assert lib.phj_index_accumulate(None, None, None, 1, None, 1, 0, None, None, None) == PHJ_ERR_INVALID


def test_python_names():
    import inspect
    import partitionedhashjoin_amd as phj
    assert "ordinals" in inspect.signature(phj.Context.build_index).parameters
    assert inspect.signature(phj.Context.build_index).parameters["ordinals"].default is False
    assert isinstance(phj.Index.ordinals, property)
    for name in ("first_rows_ptr", "first_rows", "encode", "encode_host", "accumulate", "accumulate_host"):
        assert callable(getattr(phj.Index, name)), name
    assert list(inspect.signature(phj.Index.accumulate_host).parameters) == ["self", "keys", "values"]


def cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, cwd="/tmp")


def test_cli_help_lists_lookup_as():
    r = cli("--help")
    assert r.returncode == 0 and "--lookup-as" in r.stdout
    for word in ("rows | codes |", "lookup_codes_checksum", "groups_count_checksum", "groups_sum_checksum"):
        assert word in r.stdout, word


@pytest.mark.parametrize("args,msg", [
    (("--lookup", "4", "--lookup-as", "ids"), "for option '--lookup-as' is invalid"),
    (("--lookup", "4", "--lookup-as", ""), "for option '--lookup-as' is invalid"),
    (("--lookup-as", "codes"), "give --lookup BATCHES"),
    (("--lookup-as", "rows"), "give --lookup BATCHES"),
    (("--lookup-as", "groups", "--member", "probe"), "give --lookup BATCHES"),
])
def test_cli_rejects_bad_lookup_as(args, msg):
    r = cli("--join", "no-partitioning", *args)
    assert r.returncode == 1
    assert msg in r.stdout
