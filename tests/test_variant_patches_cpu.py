"""The measured-and-dropped kernel policies live as patches of the product source under tools/variants/ (tools/variant.sh applies
them to a COPY of icp_kernels.hip).  A patch that no longer applies is a record nobody can re-measure: every one must still apply."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHES = sorted(glob.glob(os.path.join(ROOT, "tools", "variants", "*.patch")))


@pytest.mark.parametrize("patch", PATCHES, ids=[os.path.basename(p) for p in PATCHES])
def test_variant_patch_applies(patch):
    if not shutil.which("patch"):  # (as tests/test_capi_cpu.py does for fake_bounds.patch)
        return
    src = os.path.join(ROOT, "mimosa_amd", "csrc", "icp_kernels.hip")
    r = subprocess.run(["patch", "--dry-run", "-s", src, patch], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
