"""The accumulation-session entry points of include/rtw.h on a CPU-only machine: exported, struct sizes as the header states them,
NULL contexts and arguments refused with a code, and no exception crossing the C ABI (no compute calls here: tests/test_gpu_accum.py)."""
import ctypes as C
import os
import re

from raytracing_weekend_amd import abi

ACCUM = ["rtw_accum_begin", "rtw_accum_add", "rtw_accum_read", "rtw_accum_read_device", "rtw_accum_status", "rtw_accum_save",
         "rtw_accum_restore", "rtw_accum_end"]


def test_library_exports_the_session_symbols():
    lib = C.CDLL(abi.HIP_LIB)
    for name in ACCUM:
        assert hasattr(lib, name), name
        assert name in abi.HIP_SYMBOLS
    lib.rtw_abi_version.restype = C.c_int
    assert lib.rtw_abi_version() == abi.RTW_ABI_VERSION == 5
    text = open(os.path.join(abi.REPO_DIR, "include", "rtw.h")).read()
    assert re.search(r"#define RTW_ABI_VERSION 5\b", text)
    assert re.search(r"enum \{ RTW_ACCUM_ERROR = 1 \}", text) and abi.RTW_ACCUM_ERROR == 1


def test_struct_sizes_match_the_header():
    assert C.sizeof(abi.Params) == 48
    assert C.sizeof(abi.AccumInfo) == 96  # "rtw_accum_info; /* 96 B */"
    assert abi.AccumInfo.state_bytes.offset == 16 and abi.AccumInfo.params.offset == 48
    text = open(os.path.join(abi.REPO_DIR, "include", "rtw.h")).read()
    body = text[text.index("typedef struct rtw_accum_info {"):text.index("} rtw_accum_info;")]
    fields = re.findall(r"\b(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in abi.AccumInfo._fields_], fields


def test_null_context_and_arguments_are_errors_not_crashes():
    lib = abi.load_hip()
    p = abi.make_params(8, 8, 16, 2)
    info = abi.AccumInfo()
    buf = C.create_string_buffer(256)
    assert lib.rtw_accum_begin(None, C.byref(p), 0) < 0
    assert lib.rtw_accum_begin(None, None, 0) < 0
    assert lib.rtw_accum_add(None, 16, None) < 0
    assert lib.rtw_accum_read(None, buf, None) < 0
    assert lib.rtw_accum_read(None, None, None) < 0
    assert lib.rtw_accum_read_device(None, None, None) < 0
    assert lib.rtw_accum_status(None, C.byref(info)) < 0
    assert lib.rtw_accum_status(None, None) < 0
    assert lib.rtw_accum_save(None, buf, 256) < 0
    assert lib.rtw_accum_save(None, None, 0) < 0
    assert lib.rtw_accum_restore(None, buf, 256) < 0
    assert lib.rtw_accum_restore(None, None, 0) < 0
    assert lib.rtw_accum_end(None) < 0


def test_no_exception_crosses_the_session_entry_points(monkeypatch):
    """RTW_TEST_FAULT=entry:<kind> makes every entry point throw inside its guard before it looks at its arguments
    (tests/test_abi.py test_no_exception_crosses_the_c_abi): std::bad_alloc comes back as RTW_ERR_OOM, anything else as RTW_ERR_DEVICE."""
    lib = abi.load_hip()
    p = abi.make_params(8, 8, 16, 2)
    info = abi.AccumInfo()
    buf = C.create_string_buffer(256)
    for kind, want in (("bad_alloc", -5), ("runtime", -4)):
        monkeypatch.setenv("RTW_TEST_FAULT", "entry:" + kind)
        assert lib.rtw_accum_begin(None, C.byref(p), 0) == want
        assert lib.rtw_accum_add(None, 16, None) == want
        assert lib.rtw_accum_read(None, buf, None) == want
        assert lib.rtw_accum_read_device(None, None, None) == want
        assert lib.rtw_accum_status(None, C.byref(info)) == want
        assert lib.rtw_accum_save(None, buf, 256) == want
        assert lib.rtw_accum_restore(None, buf, 256) == want
        assert lib.rtw_accum_end(None) == want
    monkeypatch.delenv("RTW_TEST_FAULT")
    assert lib.rtw_accum_end(None) == -1  # back to the plain argument check
    src = open(os.path.join(abi.PKG_DIR, "csrc", "rtw_hip.hip")).read()
    ext = src[src.index('extern "C" {'):]
    for name in ACCUM:
        body = ext[ext.index("int " + name + "("):]
        assert "guarded(" in body[:body.index("\n")], name
