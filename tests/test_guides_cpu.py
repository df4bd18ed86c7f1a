"""Guide buffers and the guided denoiser without a GPU: the numpy restatement of rtw_denoise_guided against the CPU restatement
of rtw_denoise, the error paths of the two entry points, and the PFM writer of the -aov guide files."""
import ctypes as C
import os

import numpy as np

import guides_ref
import oracle
from raytracing_weekend_amd import abi


def test_restatement_with_constant_guides_is_the_colour_only_filter():
    rs = np.random.RandomState(5)
    img = rs.uniform(0, 1, (23, 37, 4)).astype(np.float32)
    for alb_v, nrm_v in ((0.0, 0.0), (0.3, -0.7)):
        alb = np.full_like(img, alb_v)
        nrm = np.full_like(img, nrm_v)
        for it, sigma in ((5, 0.5), (3, 0.2)):
            got = guides_ref.atrous_guided(img, alb, nrm, it, sigma, 0.1, 0.25)
            assert np.array_equal(got, oracle.denoise(img, it, sigma))


def test_new_entries_on_a_null_context_are_errors():
    lib = abi.load_hip()
    p = abi.make_params(8, 8, 1, 2)
    buf = (C.c_float * 256)()
    g = abi.Guides(albedo=C.addressof(buf))
    assert lib.rtw_render_guides(None, C.byref(p), C.byref(g), None) < 0
    assert lib.rtw_render_guides(None, None, None, None) < 0
    assert lib.rtw_denoise_guided(None, buf, buf, buf, None, 4, 4, 1, 0.5, 0.1, 0.1) < 0


def test_no_exception_crosses_the_new_entries(monkeypatch):
    lib = abi.load_hip()
    p = abi.make_params(8, 8, 1, 2)
    for kind, want in (("bad_alloc", -5), ("runtime", -4)):
        monkeypatch.setenv("RTW_TEST_FAULT", "entry:" + kind)
        assert lib.rtw_render_guides(None, C.byref(p), None, None) == want
        assert lib.rtw_denoise_guided(None, None, None, None, None, 1, 1, 1, 1.0, 1.0, 1.0) == want
    monkeypatch.delenv("RTW_TEST_FAULT")
    assert lib.rtw_render_guides(None, C.byref(p), None, None) == -1


def _write_pfm(path, data, stride, channels):
    lib = abi.load_host()
    lib.rtw_host_write_pfm.restype = C.c_int
    lib.rtw_host_write_pfm.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    data = np.ascontiguousarray(data, dtype=np.float32)
    h, w = data.shape[:2]
    return lib.rtw_host_write_pfm(path.encode(), data.ctypes.data, w, h, stride, channels)


def test_pfm_writer_headers_and_row_order(tmp_path):
    rs = np.random.RandomState(1)
    rgba = rs.uniform(-2, 2, (5, 7, 4)).astype(np.float32)  # row 0 = bottom row, as the frame buffer
    depth = rs.uniform(0, 900, (5, 7)).astype(np.float32)
    p3, p1 = str(tmp_path / "a_normal.pfm"), str(tmp_path / "a_depth.pfm")
    assert _write_pfm(p3, rgba, 4, 3) == 0
    assert _write_pfm(p1, depth, 1, 1) == 0
    raw3, raw1 = open(p3, "rb").read(), open(p1, "rb").read()
    hdr3, hdr1 = b"PF\n7 5\n-1.0\n", b"Pf\n7 5\n-1.0\n"
    assert raw3.startswith(hdr3) and raw1.startswith(hdr1)
    # PFM rows run bottom-up: the file's first row is buffer row 0
    assert np.array_equal(np.frombuffer(raw3[len(hdr3):], "<f4").reshape(5, 7, 3), rgba[..., :3])
    assert np.array_equal(np.frombuffer(raw1[len(hdr1):], "<f4").reshape(5, 7), depth)
    assert _write_pfm(str(tmp_path / "x.pfm"), depth, 1, 2) == -1  # RTW_ERR_INVALID_ARG: two channels is no PFM
    assert not os.path.exists(str(tmp_path / "x.pfm"))
