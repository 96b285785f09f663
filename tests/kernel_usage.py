"""The compiler's resource report of a csrc/*.hip file's kernels (CPU, hipcc cross-compile for gfx950), for
the tests that pin register, scratch and LDS budgets. A file is compiled once per process, whichever tests
ask for it: fhh_gc.hip alone takes over a minute."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _compile(src):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                            "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(ROOT, "fuzzyheavyhitters_amd", "csrc", src),
                            "-o", os.path.join(tmp, "k.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?):\s+(\S+) \[", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return usage


def resource_usage(src):
    """{mangled kernel name: {remark: value as a string}} of csrc/<src>, e.g. "VGPRs", "VGPRs Spill",
    "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]". Skips the calling test
    where there is no hipcc. The kernels' dicts are shared between callers: read them, do not change them."""
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    return dict(_compile(src))
