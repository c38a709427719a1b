"""The retained key index: what can be checked without a GPU. The four C ABI
calls and their struct are in the header, the binding's export table and the
library; the calls refuse a null context or index before touching a device;
the Python names exist; the CLI knows --lookup and refuses it beside returned
rows, aggregates, masks and several devices."""
import ctypes as C
import os
import re
import subprocess

import pytest

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")
CALLS = ["phj_index_build", "phj_index_info_get", "phj_index_lookup", "phj_index_destroy"]


def test_header_declares_the_calls_and_the_struct():
    header = open(os.path.join(ROOT, "include", "phj.h")).read()
    assert "typedef struct phj_index phj_index;" in header
    assert "typedef struct phj_index_info {" in header and "} phj_index_info;" in header
    for field in ("uint64_t rows;", "uint64_t distinct;", "uint64_t table_bytes;", "uint32_t nb, nbr, rbits, slots;"):
        assert field in header
    assert "int phj_index_build(phj_ctx *ctx, const phj_join_params *p, phj_index **out, phj_join_result *r);" in header
    assert "int phj_index_info_get(const phj_index *index, phj_index_info *out);" in header
    assert re.search(r"int phj_index_lookup\(phj_ctx \*ctx, const phj_index \*index, const int64_t \*dev_keys, "
                     r"uint32_t key_stride, uint64_t n,\s+int64_t \*out_rows, uint8_t \*out_found, "
                     r"unsigned long long \*dev_found_count\);", header)
    assert "void phj_index_destroy(phj_ctx *ctx, phj_index *index);" in header
    assert "#define PHJ_ABI_VERSION 2" in header
    assert _capi.ABI_VERSION == 2 and _capi.load().phj_abi_version() == 2


def test_struct_size_matches_the_header():
    header = open(os.path.join(ROOT, "include", "phj.h")).read()
    assert "typedef struct phj_index_info {   /* 40 B */" in header
    assert C.sizeof(_capi.IndexInfo) == 40
    assert [f[0] for f in _capi.IndexInfo._fields_] == ["rows", "distinct", "table_bytes", "nb", "nbr", "rbits", "slots"]


def test_symbols_exported_and_listed():
    L = _capi.load()
    for name in CALLS:
        assert name in _capi.EXPORTED and hasattr(L, name)
    assert len(L.phj_index_build.argtypes) == 4 and len(L.phj_index_lookup.argtypes) == 8
    assert len(L.phj_index_info_get.argtypes) == 2 and len(L.phj_index_destroy.argtypes) == 2


def test_null_context_or_index_is_invalid():
    L = _capi.load()
    r, info, h = _capi.JoinResult(), _capi.IndexInfo(), C.c_void_p()
    p = phj.nopart_params()
    assert L.phj_index_build(None, C.byref(p), C.byref(h), C.byref(r)) == _capi.PHJ_ERR_INVALID
    assert h.value is None
    assert L.phj_index_info_get(None, C.byref(info)) == _capi.PHJ_ERR_INVALID
    assert L.phj_index_lookup(None, None, None, 1, 0, None, None, None) == _capi.PHJ_ERR_INVALID
    assert L.phj_index_lookup(None, None, None, 3, 16, None, None, None) == _capi.PHJ_ERR_INVALID
    L.phj_index_destroy(None, None)   # and destroying nothing is a no-op


def test_python_names():
    for name in ("Index", "IndexInfo"):
        assert name in phj.__all__
    assert phj.IndexInfo is _capi.IndexInfo
    assert callable(phj.Context.build_index)
    for m in ("info", "lookup", "lookup_host", "close"):
        assert callable(getattr(phj.Index, m))


def test_cli_help_lists_lookup():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if "--lookup" in ln]
    assert len(line) == 1 and "BATCHES" in line[0]


def _run(tmp_path, *args):
    return subprocess.run([CLI, "--join", "no-partitioning", "-f", str(tmp_path / "x.txt"), *args],
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("bad", ["0", "-3", "many", "2.5"])
def test_cli_lookup_bad_batches(tmp_path, bad):
    r = _run(tmp_path, "--lookup", bad)
    assert r.returncode == 1
    first = r.stdout.splitlines()[0]
    assert first in ("--lookup takes 1..1000000 batches", f"the argument ('{bad}') for option '--lookup' is invalid")


@pytest.mark.parametrize("extra", [["--materialize", "on"], ["--materialize", "all"], ["--join-kind", "inner"],
                                   ["--aggregate", "totals"], ["--rows", "payloads"], ["--member", "probe"]],
                         ids=lambda e: "".join(e).lstrip("-"))
def test_cli_lookup_refused_beside_rows(tmp_path, extra):
    r = _run(tmp_path, "--lookup", "4", *extra)
    assert r.returncode == 1, extra
    assert r.stdout.splitlines()[0].startswith("--lookup returns no rows: not together with"), r.stdout[:200]


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--exchange", "local"]], ids=["gpus2", "exchange-local"])
def test_cli_lookup_runs_on_one_device(tmp_path, extra):
    r = _run(tmp_path, "--lookup", "4", *extra)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "--lookup runs on one device", r.stdout[:200]
