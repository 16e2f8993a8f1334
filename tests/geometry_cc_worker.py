"""Fresh-process check of the GSR_GRADS_COLOR_COTANGENT contract after the depth-normal term (started by
tests/_launcher.py with GSR_CHECK_COLOR_COTANGENT=1 in the environment): `l1_ssim_normal_loss` adds the term IN PLACE onto
the loss head's own cotangent buffer, so the library's pointer check cannot tell; the debugging check, which looks into
the buffer, must refuse `color_cotangent=True` with GSR_E_INVALID_ARG.  Exit status 0 = refused as expected."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsr_pkg  # noqa: E402
import scenes  # noqa: E402


def main():
    assert os.environ.get("GSR_CHECK_COLOR_COTANGENT") == "1"
    pkg = gsr_pkg.load()
    G, L = pkg.geometry_regularization, pkg._lib
    sc, ocam = scenes.grid_scene_rgbdn()
    W, H = ocam.width, ocam.height
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    cam = pkg.Camera(W, H, tuple(ocam.focal))
    rast = pkg.rasterizer.GaussianRasterizer(W, H, mode="rgbdn", device="cuda:0")
    t = [d(sc["means"]), d(sc["shs"]), d(sc["opac"].reshape(-1, 1)), d(sc["scales"]), d(sc["rots"])]
    img = rast.forward_raw(*t, cam, 0, (0.0, 0.0, 0.0))
    tgt = d(pkg.synthetic.make_target(W, H, 7))
    _, normal_term, _, vpix = G.l1_ssim_normal_loss(rast, img, tgt, cam)
    torch.cuda.synchronize()
    assert vpix[:, :, 3:].any().item(), "the term left no cotangent on channels 3..7"
    rast.backward_raw(vpix, *t, cam, 0, (0.0, 0.0, 0.0))                     # unflagged: accepted
    try:
        rast.backward_raw(vpix, *t, cam, 0, (0.0, 0.0, 0.0), color_cotangent=True)
    except L.GsrError as e:
        if e.code == L.GSR_E_INVALID_ARG and "non-zero values above the colour channels" in str(e):
            print("refused as expected:", e)
            return 0
        print("unexpected error:", e)
        return 2
    print("color_cotangent=True was accepted for a cotangent that carries the depth-normal term")
    return 1


if __name__ == "__main__":
    sys.exit(main())
