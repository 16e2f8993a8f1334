"""The point-cloud initialisation without a GPU: the two entry points exist and refuse bad arguments before anything touches
a device, the numpy reference of tests/knn_ref.py is right where the answer is known in closed form and agrees with a
KD-tree, and the Python functions check what they are given."""
import ctypes as C

import numpy as np
import pytest

import knn_ref as kr


def test_entry_points_are_declared_and_exported(pkg):
    L = pkg._lib
    lib = L.load()
    for name in ("gsr_knn_scratch_bytes", "gsr_knn_scales"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert callable(pkg.point_cloud.compute_scales) and callable(pkg.point_cloud.model_from_point_cloud)


def test_scratch_bytes(pkg):
    f = pkg._lib.load().gsr_knn_scratch_bytes
    assert f(0) == 0 and f(-1) == 0 and f(-(1 << 40)) == 0
    # 16 bytes per gathered point + one 24-byte box per 64 points
    assert f(4) == 4 * 16 + 24 and f(64) == 64 * 16 + 24 and f(65) == 65 * 16 + 48
    prev = 0
    for n in list(range(1, 300)) + [1031, 4099, 200_000, 1_000_000, (1 << 31) - 1]:
        b = f(n)
        assert b >= prev and b > 0, n
        prev = b


def test_invalid_arguments_fail_before_touching_the_gpu(pkg):
    """Every refusal of include/gsr.h, with its word in the message.  The pointers are never followed: no device needed."""
    L = pkg._lib
    lib = L.load()
    P = C.c_void_p(4096)   # "some non-null, 16-byte aligned address"
    n = 100
    nb = lib.gsr_knn_scratch_bytes(n)

    def call(n=n, points=P, order=None, ps=1.0, sd=3, scales=P, dist2=None, scratch=P, nbytes=nb):
        rc = lib.gsr_knn_scales(n, points, order, ps, sd, scales, dist2, scratch, nbytes, None)
        return rc, lib.gsr_last_error_string()

    assert call(n=0)[0] == L.GSR_OK                                # nothing to do, nothing launched
    assert call(n=0, points=None, scales=None, scratch=None, nbytes=0)[0] == L.GSR_OK
    for bad_n in (1, 2, 3):
        rc, msg = call(n=bad_n)
        assert rc == L.GSR_E_INVALID_ARG and b"n = %d" % bad_n in msg and b"4 points" in msg
    rc, msg = call(n=-5)
    assert rc == L.GSR_E_INVALID_ARG and b"negative n" in msg
    rc, msg = call(n=1 << 31, nbytes=1 << 40)
    assert rc == L.GSR_E_INVALID_ARG and b"31 bits" in msg
    for sd in (0, 2, 4, -1):
        rc, msg = call(sd=sd)
        assert rc == L.GSR_E_INVALID_ARG and b"scale_dims" in msg
    for ps in (0.0, -1.0, float("nan")):
        rc, msg = call(ps=ps)
        assert rc == L.GSR_E_INVALID_ARG and b"point_size" in msg
    for kw in (dict(points=None), dict(scales=None), dict(scratch=None)):
        rc, msg = call(**kw)
        assert rc == L.GSR_E_INVALID_ARG and b"null" in msg, kw
    for short in (0, nb - 1):
        rc, msg = call(nbytes=short)
        assert rc == L.GSR_E_INVALID_ARG and b"scratch_bytes" in msg
    rc, msg = call(scratch=C.c_void_p(4096 + 8))
    assert rc == L.GSR_E_INVALID_ARG and b"16-byte aligned" in msg


def test_reference_on_a_cubic_lattice():
    """Spacing a: every point has at least three neighbours at distance a (6 inside, 3 at a corner), none nearer."""
    for a in (0.5, 1.0, 3.0):
        g = np.stack(np.meshgrid(*([np.arange(5)] * 3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(a)
        s, d2 = kr.knn_ref(g)
        assert d2.dtype == np.float32 and s.dtype == np.float32
        assert np.array_equal(d2, np.full((125, 3), np.float32(a * a)))
        assert np.allclose(s, np.log(a), rtol=0, atol=1e-6) and s.shape == (125, 3)
        si, _ = kr.knn_ref(g, isotropic=True)
        assert si.shape == (125, 1) and np.allclose(si, np.log(a), rtol=0, atol=1e-6)
        s4, _ = kr.knn_ref(g, point_size=4.0)          # log(sqrt(md · point_size))
        assert np.allclose(s4, np.log(a) + np.log(2.0), rtol=0, atol=1e-6)
        s64, d64 = kr.knn_ref64(g)
        assert np.all(np.abs(s - s64) <= kr.scale_tolerance(s64))


def test_reference_excludes_by_index_not_by_distance():
    p = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    _, d2 = kr.knn_ref(p)
    assert np.array_equal(d2[0], [0, 0, 1]) and np.array_equal(d2[3], [1, 1, 1]) and np.array_equal(d2[4], [4, 4, 4])
    s, d2 = kr.knn_ref(np.zeros((7, 3), np.float32))   # all identical: the 1f-7 floor
    assert not d2.any() and np.allclose(s, 0.5 * np.log(1e-7), atol=1e-6)


@pytest.mark.parametrize("family", ["uniform", "blob_outliers", "planar", "collinear"])
def test_reference_agrees_with_a_kd_tree(family):
    ckdtree = pytest.importorskip("scipy.spatial").cKDTree
    p = kr.make_points(family, 1031)
    _, d2 = kr.knn_ref64(p)
    d, _ = ckdtree(p.astype(np.float64)).query(p.astype(np.float64), k=4)
    assert np.allclose(np.sqrt(d2), d[:, 1:], rtol=1e-12, atol=0)
    s, d32 = kr.knn_ref(p)
    md = (d[:, 1:] ** 2).mean(1)   # tools/train_harness.py compute_scales
    assert np.all(np.abs(s[:, 0] - np.log(np.sqrt(np.maximum(1e-7, md)))) <= kr.scale_tolerance(s[:, 0].astype(np.float64)))


def test_families_have_the_sizes_and_properties_the_gpu_tests_rely_on():
    for fam in kr.FAMILIES:
        for n in kr.SIZES[:-1]:
            p = kr.make_points(fam, n)
            assert p.shape == (n, 3) and p.dtype == np.float32 and np.isfinite(p).all()
    assert len(np.unique(kr.make_points("identical", 65), axis=0)) == 1
    assert len(np.unique(kr.make_points("duplicated", 64), axis=0)) == 32
    assert len(np.unique(kr.make_points("lattice", 257), axis=0)) == 257
    b = np.abs(kr.make_points("blob_outliers", 257)).max(1)
    assert (b > 5e3).sum() == 16 and np.median(b) < 5.0


def test_python_argument_checks(pkg):
    import torch
    pc = pkg.point_cloud
    with pytest.raises(ValueError, match="HIP"):
        pc.compute_scales(torch.zeros(10, 3))
    with pytest.raises(ValueError, match="HIP"):
        pc.compute_scales(np.zeros((10, 3), np.float32))
    with pytest.raises(ValueError, match="HIP"):
        pc.model_from_point_cloud(torch.zeros(10, 3), torch.zeros(10, 3))
    for deg in (-1, 4):
        with pytest.raises(ValueError, match=r"`max_sh_degree=%d` must be in `\[0, 3\]` range\." % deg):
            pc.model_from_point_cloud(torch.zeros(10, 3), torch.zeros(10, 3), max_sh_degree=deg)
