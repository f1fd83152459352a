"""The step kernel's LDS carve (csrc/solve_step.h: carve_lds, ds_lds_doubles) at every window the device loop takes, Wo = 1 .. 7 with
a free and a constant extrinsic (docs/wide_window.md): tests/host/wide_lds_check.hip under the address and undefined-behaviour
sanitizers.  Arrays whose lifetimes overlap occupy disjoint bytes, every array lies inside the launch's LDS size, and the total is at
most 160 KiB — at (n_pad 128, Wo 7) as well, which needed 182 848 bytes while every array had bytes of its own.  No GPU needed.

Also: include/lio_est_wide.h is bound, exported, plain C and apart from the shared ABI."""
import ctypes
import os
import re
import subprocess

from lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_carve_of_every_window_size(tmp_path):
    exe = str(tmp_path / "wide_lds_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mavx2", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "lio-mapping_amd", "csrc"), os.path.join(ROOT, "tests", "host", "wide_lds_check.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if re.match(r"\s+\d+\s+\d+\s+\d+", ln)]
    assert len(rows) == 14                                               # Wo 1 .. 7 x two extrinsic forms
    wide = [row for row in rows if row[0] == "7"]
    assert [int(row[3]) for row in wide] == [128, 128]
    assert all(int(row[5]) <= 160 * 1024 for row in rows)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_wide_header_is_bound_exported_and_apart_from_the_shared_abi():
    wide = _declared("lio_est_wide.h")
    assert set(wide) == {"lio_est_set_device_solve_limit", "lio_est_get_device_solve_limit"}
    assert set(wide) == set(capi._EST_WIDE_SIGS.keys())
    for other in sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h") and f != "lio_est_wide.h"):
        assert not set(wide) & set(_declared(other)), other
    assert not set(wide) & (set(capi._SIGS) | set(capi._TEST_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in wide:
        assert hasattr(dll, s), s


def test_wide_symbols_are_not_demanded_of_the_oracle(oracle):
    assert oracle.missing == [] and not oracle.has_ext
    for s in capi._EST_WIDE_SIGS:
        assert not hasattr(oracle.dll, s), s


def test_wide_header_is_plain_c_and_links_against_the_product(tmp_path):
    src = tmp_path / "wide.c"
    src.write_text('#include "lio_est_wide.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  if (lio_est_set_device_solve_limit(NULL, 7) != LIO_ERR_ARG) return 1;\n"
                   "  if (lio_est_get_device_solve_limit(NULL) != LIO_ERR_ARG) return 2;\n"
                   "  if (LIO_DEVICE_SOLVE_LIMIT_DEFAULT != 6 || LIO_DEVICE_SOLVE_LIMIT_MAX != 7) return 3;\n"
                   '  printf("%s\\n", lio_backend());\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "wide_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
           "-l" + libname[3:-3], "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "hip-gfx950" in r.stdout
