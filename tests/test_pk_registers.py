"""Register budgets of the packed pipeline's kernels, from the compiler's own report (no GPU needed).

A gfx950 SIMD admits min(8, 800 / (sgprs rounded up to 16, + 16)) waves of a kernel: eight up to 80 scalar registers, six
at the 106 the list kernels took before they were given a budget -- 24 waves per compute unit, three 8-wave workgroups
where the host's residency model (and the thread counts retile() chooses by it) counts on four.  The fused pass must stay
at three waves per SIMD (at most 168 vector registers) and out of scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egg_fluid_simulation_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _makefile_flags():
    """CXXFLAGS of csrc/Makefile, so that the kernels are compiled here as they are for the library"""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"CXXFLAGS\s*\??=\s*(.*)", line)
        if m:
            return m.group(1).split()
    raise AssertionError("csrc/Makefile has no CXXFLAGS line")


@pytest.fixture(scope="module")
def usage():
    if HIPCC is None:
        pytest.skip("hipcc is not installed")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", *_makefile_flags(), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "eggsim_packed.hip", "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1).split()[0]] = int(m.group(2))
    return kernels


def test_list_kernels_fit_eight_waves_per_simd(usage):
    lists = {k: v for k, v in usage.items() if k.startswith("egg_pk_lists_")}
    assert set(lists) == {"egg_pk_lists_fresh_kernel", "egg_pk_lists_stale_kernel", "egg_pk_lists_first_kernel",
                          "egg_pk_lists_stale_mid_kernel"}, sorted(usage)
    for name, u in lists.items():
        print(name, u)
        assert u["TotalSGPRs"] <= 80 and u["VGPRs"] <= 64 and u["ScratchSize"] == 0, (name, u)


def test_fused_pass_keeps_three_waves_per_simd(usage):
    u = usage["egg_pk_levexec_kernel"]
    print("egg_pk_levexec_kernel", u)
    assert u["ScratchSize"] == 0 and u["VGPRs"] <= 168, u
