"""csrc/cloud_src.h on the host — CloudSrc, the typed hand-over of a cloud between the stages: host() and device() carry pointer, count and
place, host(nullptr, 0) is the empty cloud, to_device() names the two copy kinds, and clouds_on_device() accepts an all-host, an all-device
and an empty list and throws on a mix (tests/host/cloud_src_check.cc).  No GPU: the header is host code and the program only includes HIP's
type and enum declarations."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_cloud_src_carries_place_and_refuses_a_mix(tmp_path):
    exe = str(tmp_path / "cloud_src_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                    "-I", os.path.join(ROOT, "lio-mapping_amd", "csrc"), os.path.join(HERE, "host", "cloud_src_check.cc"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("cloud_src: OK")
