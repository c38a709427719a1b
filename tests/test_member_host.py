"""Membership joins: what can be checked without a GPU. The C ABI symbol, its
two flags and its struct are in the header, the binding's export table and the
library; the call refuses a null context before touching a device; the Python
names exist; the CLI knows --member and refuses it beside returned rows."""
import ctypes as C
import os
import subprocess

import partitionedhashjoin_amd as phj
from partitionedhashjoin_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "partitionedhashjoin_amd", "phjoin")


def test_header_declares_the_call():
    header = open(os.path.join(ROOT, "include", "phj.h")).read()
    assert "int phj_join_member(phj_ctx *ctx, const phj_join_params *p, uint32_t sides," in header
    assert "#define PHJ_MEMBER_PROBE 0x1" in header and "#define PHJ_MEMBER_BUILD 0x2" in header
    assert "typedef struct phj_member_counts {" in header and "} phj_member_counts;" in header
    assert "uint64_t probe_matched;" in header and "uint64_t build_matched;" in header
    assert "#define PHJ_ABI_VERSION 2" in header
    assert _capi.ABI_VERSION == 2 and _capi.load().phj_abi_version() == 2


def test_struct_and_flags():
    assert C.sizeof(_capi.MemberCounts) == 16
    assert (_capi.MEMBER_PROBE, _capi.MEMBER_BUILD) == (1, 2)
    assert (phj.MEMBER_PROBE, phj.MEMBER_BUILD) == (1, 2) and phj.MemberCounts is _capi.MemberCounts
    for name in ("MEMBER_PROBE", "MEMBER_BUILD", "MemberCounts"):
        assert name in phj.__all__
    assert callable(phj.Context.join_member)


def test_symbol_exported_and_listed():
    L = _capi.load()
    assert "phj_join_member" in _capi.EXPORTED
    assert hasattr(L, "phj_join_member") and len(L.phj_join_member.argtypes) == 7


def test_null_context_is_invalid():
    L = _capi.load()
    r, n = _capi.JoinResult(), _capi.MemberCounts()
    p = phj.nopart_params()
    assert L.phj_join_member(None, C.byref(p), 3, None, None, C.byref(r), C.byref(n)) == _capi.PHJ_ERR_INVALID


def test_cli_help_lists_member():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    line = [ln for ln in r.stdout.splitlines() if "--member" in ln]
    assert len(line) == 1 and "probe | build | both" in line[0]


def test_cli_member_refusals(tmp_path):
    def run(*args):
        return subprocess.run([CLI, "--join", "no-partitioning", "-f", str(tmp_path / "x.txt"), *args],
                              capture_output=True, text=True, timeout=60)
    r = run("--member", "xml")
    assert r.returncode == 1 and "the argument ('xml') for option '--member' is invalid" in r.stdout
    for extra in (["--materialize", "on"], ["--materialize", "all"], ["--join-kind", "inner"],
                  ["--aggregate", "totals"], ["--rows", "payloads"]):
        r = run("--member", "both", *extra)
        assert r.returncode == 1, extra
        assert r.stdout.splitlines()[0].startswith("--member returns no rows: not together with"), (extra, r.stdout[:200])
    for extra in (["--gpus", "2"], ["--exchange", "local"]):
        r = run("--member", "probe", *extra)
        assert r.returncode == 1 and r.stdout.splitlines()[0] == "--member runs on one device", extra
