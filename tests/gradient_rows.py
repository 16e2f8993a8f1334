"""A per-Gaussian gradient criterion ("rows"): every ROW of a gradient tensor against the oracle and the float64
autograd model, not the tensor's norm.

Why: what consumes the gradients is per-Gaussian.  Adam divides each element by its own sqrt(nu), so a Gaussian whose gradient
is 1e-4 of the largest one moves as far per step as the largest one does, and `densify` thresholds each Gaussian's own
|grad means_2d|.  hip_helpers.compare_backward's relative L2 of 1e-4 over a tensor cannot see the faint rows at all: on
fuzz_scenes.sweep_scene(5) a third of the non-zero rows can be set to ZERO and the tensor still meets it (the splats deep in a
list, behind accumulated opacity: the rows the liveness trims, the saturation stop and the segment composition of the two
compositing backward kernels write).

The criterion, for one (N, k) tensor; `vis` = radii > 0, rms(ref) = root-mean-square row norm of `ref` over the visible rows,
    T_i(ref) = 1e-4 · |ref_i| + 1e-5 · rms(ref)
(1e-4: the project's gradient tolerance, SURVEY.md §8c, per row; the floor 1e-5 · rms is what the fp32 oracle alone needs against
float64 — it keeps every row down to 1e-5 of the typical one under a 100 %-error test and rows at 1e-2 of typical under a 1e-3
one).  A visible row passes by one of
    (z) it is exactly zero in the oracle AND in float64: then HIP must be exactly zero too;
    (a) |hip_i - orc_i| <= T_i(orc);
    (f) |hip_i - f64_i| <= T_i(f64);
    (b) the Gaussian's axis ratio is above 10 (`ill`, as in test_gpu_fuzz_regressions.arbitrate) and
        |hip_i - f64_i| <= 4 · |orc_i - f64_i| + T_i(f64)   (the factor of arbitrate (b) and hip_helpers.pose_ok).
Rows of `touched` — hip_helpers.blend_boundary_pixels(..., with_ids=True): Gaussians that blend into a pixel holding a (pixel,
splat) pair within 4 ulps of alpha = 1/255 — get NO tolerance of their own: they pass through (a) or (f), i.e. by agreeing with
either evaluation's decision of that pair; one that meets neither is EXEMPT, and the exempt rows may be at most 2 % of the
visible rows of that tensor (EXEMPT_CAP).  Any other failing row fails the test.  The scene's boundary pixels must themselves
be within compare_forward's bound of max(4, 2 % of the image) (boundary_pixels_ok).

Pure numpy + tests/f64_model.py; no GPU code.  The scenes both test modules use (SCENES) and their shared references
(reference) live here as well."""
import collections
from dataclasses import dataclass

import numpy as np
import torch

import f64_model as fm

NAMES = ("vmeans", "vshs", "vopacities", "vscales", "vrots")
ALL_NAMES = NAMES + ("vmeans2d",)
REL, FLOOR, ILL_RATIO, ILL_FACTOR, EXEMPT_CAP = 1e-4, 1e-5, 10.0, 4.0, 0.02
BG = (0.3, 0.1, 0.6)

Report = collections.namedtuple("Report", "name checked z a f b exempt worst")


def f64_gradients(arrays, cam, deg, mode, bg, st, vp):
    """float64 gradients of the five leaves `arrays` = (means, shs, opacities, scales, rotations) and of the projected centres,
    for the cotangent `vp`, on the discrete structure of the oracle state `st` (f64_model.render_dense): {name: (N, -1) float64}
    with the keys ALL_NAMES.

    "vmeans2d" is the oracle's `g.vmeans2d` = the reference's gstate.∇means_2d (oracle/gsr_oracle.c orc_render_bwd; render.jl
    ∇render!): the sum over the (pixel, splat) pairs of vsigma · d sigma / d (m2 - pixel), in PIXELS, with no term from the conic,
    the depth or the colour — the projected centre enters the image through sigma alone, so this IS the plain cotangent of the
    model's `m2` intermediate (m2.grad after retain_grad()); nothing is rescaled or added here.  Culled Gaussians are in no
    list: zero rows."""
    tt = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=fm.DT, requires_grad=True)  # noqa: E731
    means, shs, opac, scales, rots = arrays
    n = np.asarray(means).shape[0]
    leaves = [tt(means), tt(shs), tt(np.asarray(opac).reshape(-1)), tt(scales), tt(rots)]
    taps = {}
    img = fm.render_dense(*leaves, cam, deg, np.asarray(bg, np.float32), mode, st.values_sorted, st.ranges, st.radii, taps=taps)
    taps["m2"].retain_grad()
    (img * torch.tensor(np.asarray(vp), dtype=fm.DT)).sum().backward()
    out = {nm: leaf.grad.numpy().reshape(n, -1).copy() for nm, leaf in zip(NAMES, leaves)}
    out["vmeans2d"] = taps["m2"].grad.numpy().reshape(n, -1).copy()
    return out


def _rows(a, n):
    return np.asarray(a, np.float64).reshape(n, -1)


def row_tolerance(ref, vis):
    """T_i(ref) per row and rms(ref) over the visible rows."""
    nrm = np.linalg.norm(ref, axis=1)
    rms = float(np.sqrt((nrm[vis] ** 2).mean())) if vis.any() else 0.0
    return REL * nrm + FLOOR * rms, rms


def classify_rows(hip, orc, f64, vis, touched, ill):
    """Rule by which each row passes: 'z', 'a', 'f', 'b', 'x' (exempt: touched and none of the rules), '!' (fails) and '-' (not
    visible: not checked), as an (N,) array of one-character strings; also the per-row |hip - orc| / T_i(orc)."""
    n = vis.shape[0]
    hip, orc, f64 = _rows(hip, n), _rows(orc, n), _rows(f64, n)
    To, _ = row_tolerance(orc, vis)
    Tf, _ = row_tolerance(f64, vis)
    d_ho, d_hf, d_of = (np.linalg.norm(x, axis=1) for x in (hip - orc, hip - f64, orc - f64))
    zero_ref = ~orc.any(1) & ~f64.any(1)
    z = zero_ref & ~hip.any(1)
    a = ~zero_ref & (d_ho <= To)
    f = ~zero_ref & (d_hf <= Tf)
    b = ~zero_ref & ill & (d_hf <= ILL_FACTOR * d_of + Tf)
    rule = np.full(n, "!", dtype="<U1")
    rule[touched] = "x"
    for k, m in (("b", b), ("f", f), ("a", a), ("z", z)):   # the first rule that holds, in the order z, a, f, b
        rule[m] = k
    rule[~vis] = "-"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(To > 0, d_ho / To, np.where(d_ho > 0, np.inf, 0.0))
    return rule, ratio


def check_rows(name, hip, orc, f64, vis, touched, ill, positions=None):
    """The criterion of the module docstring on one tensor: (N, k) arrays `hip`, `orc`, `f64`, boolean (N,) `vis`, `touched`, `ill`.
    `positions` (optional, (N,) ints, -1 = unknown): the list position of each Gaussian, for the message.  Raises AssertionError
    naming every failing row (at most eight are spelt out): its list position, its norm relative to the rms and its three
    pairwise distances; and when more than EXEMPT_CAP of the visible rows are exempt.  Returns a Report: rows checked, rows passed
    by each rule, rows exempt, and the worst |hip_i - orc_i| / T_i(orc) over the rows checked."""
    vis, touched, ill = (np.asarray(x, bool) for x in (vis, touched, ill))
    n = vis.shape[0]
    hip, orc, f64 = _rows(hip, n), _rows(orc, n), _rows(f64, n)
    rule, ratio = classify_rows(hip, orc, f64, vis, touched, ill)
    count = lambda k: int((rule == k).sum())  # noqa: E731
    rep = Report(name, int(vis.sum()), count("z"), count("a"), count("f"), count("b"), count("x"),
                 float(ratio[vis].max()) if vis.any() else 0.0)
    bad = np.flatnonzero(rule == "!")
    if bad.size:
        _, rms_o = row_tolerance(orc, vis)
        rms = max(rms_o, 1e-300)
        lines = []
        for i in bad[np.argsort(-ratio[bad])][:8]:
            pos = "?" if positions is None or positions[i] < 0 else int(positions[i])
            lines.append(f"row {int(i)} (list position {pos}, axis ratio > 10: {bool(ill[i])}): |orc_i| = {np.linalg.norm(orc[i]) / rms:.2e} rms, "
                         f"|hip - orc| = {np.linalg.norm(hip[i] - orc[i]) / rms:.2e} rms, |hip - f64| = "
                         f"{np.linalg.norm(hip[i] - f64[i]) / rms:.2e} rms, |orc - f64| = {np.linalg.norm(orc[i] - f64[i]) / rms:.2e} rms, "
                         f"|hip_i| = {np.linalg.norm(hip[i]) / rms:.2e} rms")
        raise AssertionError(f"{name}: {bad.size} of {rep.checked} visible rows fail the row criterion (rms = {rms_o:.3e}):\n  "
                             + "\n  ".join(lines) + f"\n  {rep}")
    assert rep.exempt <= EXEMPT_CAP * rep.checked, f"{name}: {rep.exempt} exempt rows of {rep.checked}: more than 2 % — {rep}"
    return rep


def boundary_pixels_ok(bmask):
    """compare_forward's bound on the pixels that hold a pair on the blend boundary: at most max(4, 2 % of the image)."""
    return int(bmask.sum()) <= max(4, 0.02 * bmask.size)


def zeroable_rows(ref, vis, rule):
    """How many NON-ZERO visible rows of `ref` could be set to zero unnoticed — the blindness figure of DESIGN.md §3.
    rule "norm": the largest set (faintest rows first) whose removal keeps rel-L2 <= 1e-4 over the tensor (compare_backward);
    rule "rows": the rows with |ref_i| <= T_i(ref), each of which check_rows would accept as zero."""
    ref = _rows(ref, vis.shape[0])
    nrm = np.linalg.norm(ref, axis=1)
    live = np.sort(nrm[vis & (nrm > 0)])
    if rule == "norm":
        total = float(np.sqrt((np.asarray(ref) ** 2).sum()))
        return int((np.sqrt(np.cumsum(live ** 2)) <= 1e-4 * total).sum())
    T, _ = row_tolerance(ref, vis)
    return int((vis & (nrm > 0) & (nrm <= T)).sum())


# ---- the scenes of tests/test_gradient_rows_cpu.py and tests/test_gpu_gradient_rows.py ----
@dataclass
class RowScene:
    name: str
    arrays: tuple           # means, shs, opacities (N,), scales (activated), rotations
    cam: object
    deg: int
    mode: str
    bg: tuple
    vp: np.ndarray          # the cotangent (H, W, C)
    order: np.ndarray = None   # one-tile scenes: order[p] = Gaussian at list position p
    stop: int = None           # walled scenes: the walk ends after `stop` entries at every pixel
    length: int = None         # one-tile scenes: entries of THE list


CELLS = {101: ("rgb", 3, 64, 48, 300), 102: ("rgb", 0, 64, 48, 300), 103: ("rgbd", 1, 80, 64, 400),
         104: ("rgbdn", 2, 64, 48, 300), 106: ("rgb", 2, 64, 40, 500)}   # test_forward_backward_vs_oracle without 200 x 120
SWEEP, EDGE = tuple(f"sweep-{c}" for c in range(12)), tuple(f"edge-{c}" for c in range(6))
ONE_TILE = ("tile-65", "tile-1025", "tile-2049", "tile-1025-rgbdn", "walled-1000-64", "walled-2500-1025")
SCENES = tuple(f"cell-{s}" for s in CELLS) + SWEEP + EDGE + ("needle-1",) + ONE_TILE
PRECISION_SCENES = ("sweep-5", "edge-2", "needle-1", "walled-2500-1025")
FAULT_SCENES = ("sweep-5", "edge-2", "walled-2500-1025")


def build_scene(pkg, name):
    import fuzz_scenes
    import list_scenes as ls
    from oracle.oracle import Camera
    kind, *rest = name.split("-")
    C = {"rgb": 3, "rgbd": 5, "rgbdn": 8}
    if kind == "cell":
        seed = int(rest[0])
        mode, deg, W, H, n = CELLS[seed]
        s = pkg.synthetic.make_scene(n, W, H, deg, seed, sigma_px=4.0)
        R, t = pkg.synthetic.view_pose(3)
        vp = np.random.default_rng(seed).standard_normal((H, W, C[mode])).astype(np.float32)
        return RowScene(name, (s.means, s.shs, s.opacities, s.scales, s.rotations), Camera(W, H, s.focal, R=R, t=t), deg, mode, BG, vp)
    if kind in ("sweep", "edge", "needle"):
        fs = getattr(fuzz_scenes, kind + "_scene")(pkg, int(rest[0]))
        return RowScene(name, (fs.means, fs.shs, fs.opac, fs.scales, fs.rots), fs.cam, fs.deg, fs.mode, fs.bg, fs.cotangent())
    if kind == "tile":
        L, mode = int(rest[0]), rest[1] if len(rest) > 1 else "rgb"
        sc, stop = ls.single_tile_scene(L, 7), None
    else:
        L, stop, mode = int(rest[0]), int(rest[1]), "rgb"
        sc = ls.walled_scene(L, stop, 11, deg=int(rest[2][3:]) if len(rest) > 2 else 0)   # ("walled-L-stop-deg2")
    vp = np.random.default_rng(1000 + L).standard_normal((16, 16, C[mode])).astype(np.float32)
    return RowScene(name, sc.args, sc.cam, sc.deg, mode, BG, vp, sc.order, stop, L)


Reference = collections.namedtuple("Reference", "sc st orc f64 vis touched ill positions bmask")
_references = {}


def reference(pkg, orc, name):
    """Scene, oracle state, oracle and float64 gradients ({name: (N, k) float64} over ALL_NAMES), `vis`, `touched`, `ill`, the list
    positions (one-tile scenes; else None) and the boundary-pixel mask of one scene of SCENES: computed once, shared, read-only."""
    if name not in _references:
        from hip_helpers import blend_boundary_pixels
        sc = build_scene(pkg, name)
        means, shs, opac, scales, rots = sc.arrays
        st = orc.forward(means, shs, opac, scales, rots, sc.cam, sc.deg, background=sc.bg, mode=sc.mode)
        g = oracle_gradients(orc, sc, st)
        f64 = f64_gradients(sc.arrays, sc.cam, sc.deg, sc.mode, sc.bg, st, sc.vp)
        n = means.shape[0]
        bmask, _, ids = blend_boundary_pixels(st, opac, sc.cam.width, sc.cam.height, with_ids=True)
        touched = np.zeros(n, bool)
        touched[list(ids)] = True
        s = np.abs(np.asarray(scales, np.float64))
        ill = s.max(1) / np.maximum(s.min(1), 1e-30) > ILL_RATIO
        positions = None
        if sc.order is not None:
            positions = np.full(n, -1, np.int64)
            positions[sc.order] = np.arange(sc.order.size)
        for a in list(g.values()) + list(f64.values()) + [sc.vp, st.values_sorted, st.ranges, st.radii]:
            a.setflags(write=False)
        _references[name] = Reference(sc, st, g, f64, st.radii > 0, touched, ill, positions, bmask)
    return _references[name]


def oracle_gradients(orc, sc, st, deterministic=True):
    means, shs, opac, scales, rots = sc.arrays
    n = means.shape[0]
    g = orc.backward(st, sc.vp, means, shs, opac, scales, rots, sc.cam, sc.deg, background=sc.bg, deterministic=deterministic)
    return {nm: _rows(a, n) for nm, a in zip(ALL_NAMES, (g.vmeans, g.vshs, g.vopacities, g.vscales, g.vrots, g.vmeans2d))}


def check_scene(ref, hip, names=ALL_NAMES, label=""):
    """check_rows on every tensor of `names` of one scene (`hip`: {name: (N, k)}), after the scene's own condition: its boundary
    pixels are a handful.  Prints one report line per tensor and returns {name: Report}."""
    assert boundary_pixels_ok(ref.bmask), (ref.sc.name, int(ref.bmask.sum()), ref.bmask.size)
    reports = {}
    for nm in names:
        rep = check_rows(f"{ref.sc.name}{label} {nm}", hip[nm], ref.orc[nm], ref.f64[nm], ref.vis, ref.touched, ref.ill, ref.positions)
        print(f"rows {rep.name}: checked {rep.checked}, z {rep.z}, a {rep.a}, f {rep.f}, b {rep.b}, exempt {rep.exempt}, "
              f"worst |hip - orc| / T = {rep.worst:.3f}")
        reports[nm] = rep
    return reports
