"""gsr_forward_scored and gsr_contribution_mask on guarded arenas (tests/guarded.py) at both skews and both guard fills: nothing
outside the three score arrays / the mask is written, the inputs are unchanged, and the results are the same bits in every
placement.  Under skew "worst" max_weight starts at 4 mod 16 and hits / weight_sum at 8 mod 16: the entry points may ask for no more.
Then one scored forward on a handle created under GSR_DEBUG_GUARD=1: gsr_debug_check_guards stays clean."""
import numpy as np
import pytest
import torch

import definition_ref as dr
from guarded import placements
from test_gpu_definition import hip_run
from test_gpu_guarded_handle import debug_guard, guards_ok

pytestmark = pytest.mark.gpu

I32, I64, U8 = torch.int32, torch.int64, torch.uint8


class Placed:
    """Three placed arrays as the `scores` argument of forward_raw."""

    def __init__(self, L, bits, hits, q):
        self.L, self.bits, self.hits, self.q, self.n_views = L, bits, hits, q, 0

    def as_struct(self, n, device):
        assert n == self.bits.numel()
        return self.L.Scores(self.bits.data_ptr(), self.hits.data_ptr(), self.q.data_ptr(), 0, 0)


@pytest.mark.parametrize("name", ["ragged", "deep-276"])
def test_scored_forward_and_mask_on_guarded_buffers(pkg, name):
    L, lib = pkg._lib, pkg._lib.load()
    defn = dr.definition(pkg, name)
    run = hip_run(pkg, defn, True)
    n = int(run.t[0].shape[0])
    ref = None
    for P in placements(1 << 20, "cuda"):
        tag = f"{P.skew}/{P.fill}"
        # (guard values in range for a score: an over-read would change a mask byte, not an address)
        bits = P.place("max_weight", (n,), I32, role="inout", guard=(0, 1))
        hits = P.place("hits", (n,), I64, align=8, role="inout", guard=(0, 1))
        q = P.place("weight_sum", (n,), I64, align=8, role="inout", guard=(0, 1))
        masks = [P.place(f"valid_{r}", (n,), U8) for r in range(3)]
        if P.skew == "worst":
            assert bits.data_ptr() % 16 == 4 and hits.data_ptr() % 16 == 8 and q.data_ptr() % 16 == 8 and masks[0].data_ptr() % 2 == 1
        for m in masks:
            m.fill_(0xFF)
        img = run.rast.forward_raw(*run.t, run.camera, run.deg, run.bg, scores=Placed(L, bits, hits, q)).clone()
        thr = (0.01, 0.25, 3.0)
        rcs = [lib.gsr_contribution_mask(n, r, thr[r], bits.data_ptr(), hits.data_ptr(), q.data_ptr(), masks[r].data_ptr(),
                                         torch.cuda.current_stream().cuda_stream) for r in range(3)]
        assert rcs == [0, 0, 0], (tag, lib.gsr_last_error_string().decode())
        torch.cuda.synchronize()
        assert P.check() == [], (tag, P.check())
        P.assert_inputs_unchanged()
        got = dict(img=img, bits=bits.clone(), hits=hits.clone(), q=q.clone(), **{f"m{r}": masks[r].clone() for r in range(3)})
        if ref is None:
            ref = got
            assert int(hits.sum()) > 0
            b, h, w = bits.cpu().numpy().view(np.float32), hits.cpu().numpy(), q.cpu().numpy()
            assert np.array_equal(got["m0"].cpu().numpy(), (b >= np.float32(0.01)).astype(np.uint8))
            assert np.array_equal(got["m1"].cpu().numpy(), (w >= int(np.ceil(0.25 * 2.0 ** 24))).astype(np.uint8))
            assert np.array_equal(got["m2"].cpu().numpy(), (h >= 3).astype(np.uint8))
            continue
        for k in got:
            assert torch.equal(got[k], ref[k]), (tag, k)
    run.rast.close()


def test_scored_forward_under_debug_guard(pkg):
    defn = dr.definition(pkg, "deep-276")
    out = []
    for on in (False, True):
        with debug_guard(on):
            run = hip_run(pkg, defn, True)
            sc = pkg.contribution.ContributionScores(int(run.t[0].shape[0]), "cuda")
            for fo in (False, True):
                run.rast.forward_raw(*run.t, run.camera, run.deg, run.bg, forward_only=fo, scores=sc)
            guards_ok(pkg, run.rast)
            out.append((sc.bits.clone(), sc.hits.clone(), sc.q.clone()))
            run.rast.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert int(out[0][1].sum()) > 0
