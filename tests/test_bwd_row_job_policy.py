"""CPU: gsr_policy_bwd_row_job (include/gsr_policy.h) — how many single-wave workgroups the row-independent job of the :rgb
backward's tile-walk launch gets and how many Gaussians each takes.  What the kernel relies on (bwd_row_job.h walks
[w * slice, min(n, (w + 1) * slice)) in trips of 64 and never looks at n_wg): the slices cover every Gaussian, none is empty, a
slice is a multiple of 64.  What the rule promises: 256 .. 2048 Gaussians per workgroup, about 512 workgroups in between."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P(pkg, tmp_path_factory):
    """The policy layer built with g++ alone, as tests/test_policy.py builds it."""
    L = pkg._lib
    out = tmp_path_factory.mktemp("row_job_policy") / "libgsr_policy_only.so"
    src = os.path.join(ROOT, "gaussiansplatting.jl_amd", "csrc", "gsr_policy.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", src, "-o", str(out)], check=True)
    return L.bind_policy(C.CDLL(str(out))), L


def job(P, n):
    lib, L = P
    cfg, out = L.PolicyConfig(), L.BwdRowJob(7, 7)
    lib.gsr_policy_config_init(C.byref(cfg), 1920, 1080, 0, -1)
    lib.gsr_policy_bwd_row_job(C.byref(cfg), n, C.byref(out))
    return int(out.n_wg), int(out.slice)


def test_no_gaussians_no_job(P):
    assert job(P, 0) == (0, 0) and job(P, -5) == (0, 0)


NS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2000, 100_000, 131_071, 131_072, 131_073, 1_000_000, 1_048_576, 1_048_577,
      4_000_000, 2 ** 31 - 1]


@pytest.mark.parametrize("n", NS)
def test_slices_cover_every_gaussian_once(P, n):
    n_wg, slc = job(P, n)
    assert slc % 64 == 0 and 256 <= slc <= 2048
    assert n_wg * slc >= n, "every Gaussian is in a slice"
    assert (n_wg - 1) * slc < n, "no workgroup has an empty slice"
    assert n_wg == -(-n // slc)


def test_the_sizes_the_rule_names(P):
    assert job(P, 1) == (1, 256)
    assert job(P, 257) == (2, 256)
    assert job(P, 100_000) == (391, 256)          # config 2: four trips per workgroup, not one workgroup per 2048
    assert job(P, 1_000_000) == (505, 1984)       # the headline: about 512 workgroups of 31 trips
    assert job(P, 4_000_000) == (1954, 2048)      # beyond 1 M: more workgroups, not longer ones
    sizes = [job(P, n)[1] for n in (1, 1000, 131_072, 131_073, 500_000, 1_048_576, 1_048_577, 10_000_000)]
    assert sizes == sorted(sizes), "a slice never shrinks as the scene grows"


def test_the_library_exports_the_same_function(P, pkg):
    lib, L = P
    full = L.load()
    cfg = L.PolicyConfig()
    full.gsr_policy_config_init(C.byref(cfg), 1920, 1080, 0, -1)
    for n in NS:
        out = L.BwdRowJob()
        full.gsr_policy_bwd_row_job(C.byref(cfg), n, C.byref(out))
        assert (int(out.n_wg), int(out.slice)) == job(P, n), n
