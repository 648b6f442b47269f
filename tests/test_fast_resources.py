"""The fast replay kernel's register budget, read from the kernel metadata of the gfx950 code
object inside cadence_amd/libcdr.so (no device needed): k_replay_fast<false> runs four waves
per SIMD only at <= 128 VGPRs, and neither instantiation may touch scratch — a spilled build
of this kernel once ran 3.3x slower.  Numbers from the metadata notes only."""
import os
import re
import subprocess

import pytest

from cadence_amd import abi

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FAST = "_Z13k_replay_fastILb0EEv10cdr_launch"
FAST_TASKS = "_Z13k_replay_fastILb1EEv10cdr_launch"


def lib_path():
    return os.path.join(os.path.dirname(os.path.abspath(abi.__file__)), "libcdr.so")


def code_objects(lib, tmp):
    """The gfx950 code objects of the library's fat binary section: one bundle per translation
    unit, each unbundled the way tools/isa_execz_lint.py unbundles an object's."""
    fb = os.path.join(tmp, "lib.fatbin")
    # (with no output file objcopy would rewrite the library in place, under the processes that have it mapped)
    subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fb, lib, os.path.join(tmp, "lib.copy")], check=True)
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    for i, a in enumerate(starts):
        part = os.path.join(tmp, f"bundle{i}.fatbin")
        with open(part, "wb") as f:
            f.write(data[a:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = os.path.join(tmp, f"bundle{i}.co")
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                        "--targets=" + TARGET, "--output=" + co], check=True)
        if os.path.getsize(co):
            yield co


def kernel_metadata(co):
    """{kernel name: {key: value}} of the top-level scalar fields of amdhsa.kernels."""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = [], None
    for line in out.splitlines():
        m = re.match(r"^  - (\.\w+):\s*(.*)$", line)
        if m:  # a new entry of a top-level list (amdhsa.kernels)
            cur = {}
            kernels.append(cur)
        else:
            m = re.match(r"^    (\.\w+):\s*(.*)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
    return {k[".name"]: k for k in kernels if ".name" in k}


@pytest.fixture(scope="module")
def fast_kernels(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fast_resources"))
    found = {}
    for co in code_objects(lib_path(), tmp):
        md = kernel_metadata(co)
        found.update({n: md[n] for n in (FAST, FAST_TASKS) if n in md})
    assert set(found) == {FAST, FAST_TASKS}, sorted(found)
    return found


def test_fast_kernel_fits_four_waves_per_simd(fast_kernels):
    k = fast_kernels[FAST]
    print({f: k[f] for f in (".vgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count")})
    assert int(k[".vgpr_count"]) <= 128
    assert int(k[".private_segment_fixed_size"]) == 0
    assert int(k[".vgpr_spill_count"]) == 0


def test_fast_tasks_kernel_has_no_scratch(fast_kernels):
    k = fast_kernels[FAST_TASKS]
    print({f: k[f] for f in (".vgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count")})
    assert int(k[".private_segment_fixed_size"]) == 0
    assert int(k[".vgpr_spill_count"]) == 0
