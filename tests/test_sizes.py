"""The size table of the handle's buffers (csrc/gsr_sizes.h) against the closed forms, written out here.  The header includes no
HIP header: a stand-alone host program around it is built with g++ alone — once plainly, once with AddressSanitizer and UBSan
(run directly: its own main, nothing preloaded) — and prints every size for the edge cases of the two functions: 0, 1 and the
neighbours of a 256-Gaussian block; no instance, one, and a slot count equal to and beyond an odd instance count."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "gsr_sizes.h"
int main() {
    const size_t ns[] = {0, 1, 255, 256, 257};
    const uint64_t ds[][2] = {{0, 0}, {1, 1}, {1031, 1031}, {1031, 1500}};
    const int modes[] = {3, 5, 8};
    for (int C : modes) {
        for (size_t n : ns) {
            const gsr_gaussian_bytes b = gsr_sizes_per_gaussian(n, C, 12 * ((n + 255) / 256));
            printf("G %zu %d %zu %zu %zu %zu %zu %zu\n", n, C, b.geo, b.radii, b.block, b.gnormal, b.vmean2d, b.pose_part);
        }
        for (auto& d : ds) {
            const gsr_instance_bytes b = gsr_sizes_per_instance(d[0], d[1], C), r = gsr_sizes_reserve_instances(d[0], C);
            printf("I %zu %zu %d %zu %zu %zu %zu\n", (size_t)d[0], (size_t)d[1], C, b.values_sorted, b.stream, b.s3, b.rows);
            printf("R %zu %d %zu %zu %zu %zu\n", (size_t)d[0], C, r.values_sorted, r.stream, r.s3, r.rows);
        }
    }
}
"""


@pytest.fixture(scope="module", params=[(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def printed(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sizes")
    (d / "sizes_main.cpp").write_text(PROGRAM)
    exe = d / "sizes_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *request.param,
                    "-I", os.path.join(ROOT, "gaussiansplatting.jl_amd", "csrc"), str(d / "sizes_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    rows = [line.split() for line in out.stdout.splitlines()]
    return {kind: [tuple(int(x) for x in r[1:]) for r in rows if r[0] == kind] for kind in "GIR"}


def test_per_gaussian_sizes(printed):
    assert len(printed["G"]) == 15
    for n, C, geo, radii, block, gnormal, vmean2d, pose_part in printed["G"]:
        nn = max(n, 1)
        assert geo == nn * 64 and radii == nn * 4
        assert block == ((n + 255) // 256 + 1) * 4                     # bsum, bpre, bvis: each
        assert gnormal == (nn * 16 if C > 5 else 0)
        assert vmean2d == n * 8
        assert pose_part == 12 * ((n + 255) // 256) * 4                # the float count it was given, in bytes


def test_per_instance_sizes(printed):
    assert len(printed["I"]) == 12
    for D, slots, C, values_sorted, stream, s3, rows in printed["I"]:
        assert values_sorted == D * 4 and stream == D * 16             # s0, s1, s2: each
        assert s3 == (D * 16 if C > 3 else 0)
        assert rows == slots * 64


def test_reserve_sizes_rows_for_one_and_a_half_slots_per_instance(printed):
    assert len(printed["R"]) == 12
    for D, C, values_sorted, stream, s3, rows in printed["R"]:
        assert (values_sorted, stream, s3) == (D * 4, D * 16, D * 16 if C > 3 else 0)
        assert rows == D * 96                                          # exactly, for an odd D too (1031)
