"""CPU suite of the photometric window batch (mh_photo_factor_linearize_batch[_async]): the ABI surface, the argument
checks that need no device, and the C++ host mirror's compilation.  No GPU."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_FUNCS = ["mh_photo_factor_linearize_batch", "mh_photo_factor_linearize_batch_async"]


def _header():
    return open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()


def test_header_declares_the_batch_and_its_limit():
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for fn in BATCH_FUNCS:
        assert re.search(r"\bint\s+" + fn + r"\s*\(", code), fn
    m = re.search(r"#define\s+MH_PHOTO_MAX_BATCH\s+(\d+)", code)
    assert m and int(m.group(1)) == 256
    # the contract is written down where the functions are declared
    assert "bit-identical" in src and "MH_PHOTO_MAX_BATCH" in src


def test_library_exports_the_batch():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    missing = [f for f in BATCH_FUNCS if not hasattr(L, f)]
    assert not missing, missing
    assert set(BATCH_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    assert callable(capi.photo_linearize_batch) and callable(capi.photo_linearize_batch_async)


def test_null_and_empty_batches_are_rejected_without_a_device():
    from mimosa_amd import capi
    L = capi.load()
    one = (C.c_double * 9)()
    out = (capi.PhotoResult * 1)()
    assert L.mh_photo_factor_linearize_batch(None, 1, one, one, None, None, out) == capi.MH_ERR_INVALID_ARG
    assert L.mh_photo_factor_linearize_batch_async(None, 1, one, one, None, None) == capi.MH_ERR_INVALID_ARG
    empty = (C.c_void_p * 1)()
    assert L.mh_photo_factor_linearize_batch(empty, 0, one, one, None, None, out) == capi.MH_ERR_INVALID_ARG
    assert L.mh_photo_factor_linearize_batch_async(empty, 0, one, one, None, None) == capi.MH_ERR_INVALID_ARG
    assert L.mh_photo_factor_linearize_batch(empty, 1, one, one, None, None, out) == capi.MH_ERR_INVALID_ARG  # a NULL factor
    assert b"factor" in (L.mh_last_error(None) or b"")


def test_host_mirror_batch_driver_compiles_against_gtsam_sig(tmp_path):
    """photometric.hpp's linearizeBatch / linearizeBatchAsync and tests/cpp/photo_batch.cpp build warning-free against
    host/gtsam_sig and link with the library."""
    from mimosa_amd import build
    lib = build.build()
    exe = str(tmp_path / "photo_batch")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I",
                           os.path.join(ROOT, "mimosa_amd", "host", "gtsam_sig"), os.path.join(ROOT, "tests", "cpp", "photo_batch.cpp"),
                           "-o", exe, "-L", os.path.dirname(lib), "-lmimosa_hip", "-lpthread", f"-Wl,-rpath,{os.path.dirname(lib)}"])
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "mimosa_amd", "host", "mimosa_hip", "photometric.hpp")).read()
    assert "static std::vector<std::shared_ptr<GaussianFactor>> linearizeBatch(const std::vector<Ptr> & factors, const Values & c)" in src
    assert "static void linearizeBatchAsync(" in src
