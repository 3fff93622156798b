"""CPU: the float64 instantiation of the sixteen-lane kernel (dexr_tuning.kernel_f64) -- its C-ABI and its code objects.

The tuning field and the query are part of the public header, the library exports the query and the Python mirror carries
both; every float64 dexr_wide_kernel the build leaves in build/ runs without spilled VGPRs and without scratch (read from the
code-object notes with tools/codeobj_resources.py, as profiles/r07_codeobj_resources.txt records them)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from testutil import REPO
from dex_retargeting_amd import _build, _lib

sys.path.insert(0, os.path.join(REPO, "tools"))
import codeobj_resources  # noqa: E402

F64_OBJECTS = ["dexr_wide_d_16.o", "dexr_wide_d_24.o", "dexr_wide_d_m_16.o", "dexr_wide_d_mc_16.o"]


def _header():
    with open(os.path.join(REPO, "include", "dexr.h")) as f:
        return f.read()


def test_header_declares_kernel_f64_and_its_query():
    h = _header()
    m = re.search(r"typedef struct dexr_tuning \{(.*?)\} dexr_tuning;", h, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [ln.strip() for ln in body.split(";") if ln.strip()]
    assert fields[-1] == "int32_t kernel_f64", fields[-3:]
    assert re.search(r"int dexr_model_kernel_f64\(const dexr_model\* m, int32_t\* family, int32_t\* bucket\);", h)


def test_python_mirror_and_export():
    assert _lib.Tuning._fields_[-1] == ("kernel_f64", ctypes.c_int32)
    assert "dexr_model_kernel_f64" in _lib.EXPORTS
    assert os.path.exists(_lib.LIB_PATH), "build() leaves libdexr.so in the package"
    # (the dynamic symbol table, read without loading the library: loading it here would pick the HIP runtime of the process
    # before torch does)
    syms = subprocess.run([os.path.join(codeobj_resources.LLVM, "llvm-readelf"), "--dyn-syms", "-W", _lib.LIB_PATH],
                          capture_output=True, text=True, check=True).stdout
    assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+dexr_model_kernel_f64$", syms, re.M)


@pytest.mark.parametrize("obj", F64_OBJECTS)
def test_float64_wide_kernels_have_no_spills_and_no_scratch(obj):
    path = os.path.join(_build.BUILD, obj)
    assert os.path.exists(path), f"{obj} is not in {_build.BUILD}: build() compiles the float64 instantiation"
    ks = codeobj_resources.kernels_of(path)
    names = codeobj_resources.demangle([k["name"] for k in ks])
    wide = [(k, n) for k, n in zip(ks, names) if "dexr::dexr_wide_kernel<" in n]
    assert len(wide) == 1, names
    k, name = wide[0]
    targs = re.search(r"dexr::dexr_wide_kernel<([^>]*)>", name).group(1).replace(" ", "").split(",")
    assert targs[3:] == ["false", "true"], name  # <NMAX, MIMIC, MODCHOL, SPRINT = false, F64 = true>
    assert int(k["vgpr_spill_count"]) == 0, (name, k)
    assert int(k["private_segment_fixed_size"]) == 0, (name, k)
