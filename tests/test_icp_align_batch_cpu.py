"""CPU: the ABI additions of the batched alignment — mh_icp_align_batch[_async], mh_icp_align_batch_wait and
mh_icp_relocalise_batch — in the header, the library and the Python binding, and their refusals that need no device.

The batch's step kernel runs the functions of mimosa_amd/csrc/align_device.hpp per member, unchanged (tests/cpp/align_step.cpp holds
them under g++); what the call adds on the host — the per-member argument blocks and the "every member has stopped" fold — lives in
chain_api.hip, not in a header the device shares, so there is no stand-alone host program for it: the GPU suite
(test_gpu_icp_align_batch.py) holds every member to mh_icp_align bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["mh_icp_align_batch", "mh_icp_align_batch_async", "mh_icp_align_batch_wait", "mh_icp_relocalise_batch"]


def header():
    return open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()


def test_header_declares_the_four_functions_and_the_binding_lists_them():
    from mimosa_amd import capi
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", src))
    for f in FUNCS:
        assert f in declared, f
        assert f in capi.EXPORTS, f
    assert "#define MH_ABI_VERSION 3" in header()  # entry points were added, nothing that exists changed


def test_library_builds_for_gfx950_with_the_step_kernel():
    from mimosa_amd import build
    lib = build.build()
    L = C.CDLL(lib)
    for f in FUNCS:
        assert hasattr(L, f), f
    assert L.mh_abi_version() == 3
    assert build.ARCH == "gfx950"
    # the kernel is in the gfx950 code object the library carries: its name is in the bundle's symbol table
    names = subprocess.run(["strings", "-a", lib], capture_output=True, text=True, check=True).stdout
    assert "icp_align_batch_step_kernel" in names and "icp_align_step_kernel" in names


def test_batch_maximum_in_c_equals_the_binding(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "mx.c"
    src.write_text('#include <stdio.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%d %d\\n", (int)MH_ALIGN_BATCH_MAX, (int)MH_RELOC_MAX_REFINE); return 0; }\n')
    exe = str(tmp_path / "mx")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [capi.MH_ALIGN_BATCH_MAX, capi.MH_RELOC_MAX_REFINE]
    assert capi.MH_ALIGN_BATCH_MAX == 16 >= capi.MH_RELOC_MAX_REFINE  # every candidate of a relocalisation fits one batch


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    I, z, g = np.eye(3).ravel().copy(), np.zeros(3), np.array([0.0, 0.0, -1.0])
    cfg = capi.make_align_config()
    out = (capi.AlignResult * 2)()
    none = (C.c_void_p * 2)(None, None)
    for fn in (L.mh_icp_align_batch, L.mh_icp_align_batch_async):
        for handles, B in ((None, 1), (none, 2), (none, 0), (none, capi.MH_ALIGN_BATCH_MAX + 1)):
            rc = fn(handles, B, capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), out)
            assert rc == capi.MH_ERR_INVALID_ARG
            assert b"mh_icp_align_batch" in L.mh_last_error(None)
    assert L.mh_icp_align_batch_wait(None) == capi.MH_ERR_INVALID_ARG
    assert b"mh_icp_align_batch_wait" in L.mh_last_error(None)
    rcfg, res = capi.make_reloc_config(), capi.RelocResult()
    rc = L.mh_icp_relocalise_batch(None, none, 2, capi._p(I), capi._p(z), 1, capi._p(g), C.byref(rcfg), C.byref(res))
    assert rc == capi.MH_ERR_INVALID_ARG and b"NULL" in L.mh_last_error(None)


def test_python_surface():
    import inspect
    from mimosa_amd import capi
    assert list(inspect.signature(capi.align_batch).parameters) == ["factors", "poses", "cfg", "g_unit", "wait"]
    assert inspect.signature(capi.align_batch).parameters["wait"].default is True
    assert inspect.signature(capi.ICPFactor.relocalise).parameters["batch"].default is False
    assert hasattr(capi.AlignBatchCall, "wait") and hasattr(capi.ICPFactor, "release_reloc_work")
    cfg = capi.make_align_config()
    with pytest.raises(ValueError):  # before the library is asked: there is no factor to take the context from
        capi.align_batch([], [], cfg)
    with pytest.raises(ValueError):
        capi.align_batch([object()], [], cfg)
